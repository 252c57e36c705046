"""The channel's fading paths (include/pirip_hip.h section O, fading) without a GPU: the symbols, the binding's argument
and the CLI option are there and every limit answers before a device is looked for; a fade's table is its definition; the model on a
case worked by hand; the model's mean power and the autocorrelation of its scatter part; the inputs of tests/test_air_fade.py stay clear
of the quantiser's ties and reach what they claim; and the reason for the feature: the oracle demodulator and the reference chain on the
model's fading output."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import airref
import airshapes as sh
import driftref
import faderef
import fadeshapes as fs
import muxshapes as ms
import sigutil

FADE_SYMBOLS = ("pirip_hip_air_create_fade", "pirip_hip_air_fade_table")
BAD_ARG, UNSUPPORTED = -1, -6


def test_symbols_binding_cli_and_abi(built_lib):
    import pirip_amd
    out = subprocess.run(["nm", "-D", "--defined-only", pirip_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    hdr = open(os.path.join(ms.ROOT, "include", "pirip_hip.h")).read()
    for n in FADE_SYMBOLS:
        assert n in exported and hasattr(built_lib, n) and n + "(" in hdr, n
    assert "pirip_air_fade" in hdr and "#define PIRIP_HIP_ABI_VERSION 2" in " ".join(hdr.split())
    abi = C.c_int(0)
    assert built_lib.pirip_hip_abi(C.byref(abi), None, None) == 0 and abi.value == 2
    assert [f[0] for f in pirip_amd.AirFade._fields_] == ["path", "doppler_millihz", "rice_k", "key"] and C.sizeof(pirip_amd.AirFade) == 16
    assert inspect.signature(pirip_amd.HipAir).parameters["fades"].default is None
    assert callable(pirip_amd.air_fade_table)
    # Hz as a float, rounded to whole millihertz; tuples, dicts and structs alike
    f = pirip_amd.air_fade((3, 20.0004, 4.0, 7))
    assert (f.path, f.doppler_millihz, f.rice_k, f.key) == (3, 20000, 4.0, 7)
    f = pirip_amd.air_fade(dict(path=1, doppler_hz=0.0126))
    assert (f.path, f.doppler_millihz, f.rice_k, f.key) == (1, 13, 0.0, 0)
    assert pirip_amd.air_fade(f) is f
    tool = os.path.join(ms.BIN, "air_channels")
    usage = subprocess.run([tool, "--help"], capture_output=True, text=True).stderr
    assert "--fade path,doppler_millihz,rice_k[,key]" in usage
    # the fields but rice_k are integers: refused as arguments, before any file or device
    assert subprocess.run([tool, "--fs", "240000", "--fade", "0,20.5,0", "a", "--", "b"], capture_output=True).returncode == 1
    assert subprocess.run([tool, "--fs", "240000", "--fade", "0,20", "a", "--", "b"], capture_output=True).returncode == 1


def _create(L, fades, nfades=None, npaths=2, Fs=240000, null=False):
    import pirip_amd
    arr = (pirip_amd.AirPathEx * npaths)()
    for i in range(npaths):
        arr[i] = pirip_amd.AirPathEx(0, 0, 10 * i, 0, 1.0, 0)
    farr = (pirip_amd.AirFade * max(len(fades), 1))(*[pirip_amd.AirFade(*f) for f in fades])
    h = C.c_void_p()
    rc = L.pirip_hip_air_create_fade(Fs, 1, 1, 1, 1, npaths, C.addressof(arr), len(fades) if nfades is None else nfades,
                                     None if null else C.addressof(farr), None, 1, 0, -1, C.byref(h))
    if rc == 0:
        L.pirip_hip_air_destroy(h)
    return rc


def test_every_limit_answers_before_a_device_is_looked_for(built_lib):
    """both sides of every PIRIP_ERR_BAD_ARG / PIRIP_ERR_UNSUPPORTED of pirip_hip_air_create_fade; the good side gets as far as the device
    (a handle, or PIRIP_ERR_NO_DEVICE here)"""
    L = built_lib
    good = lambda rc: rc not in (BAD_ARG, UNSUPPORTED)
    for Fs in (240000, 1 << 24, 1025):
        lim = 1000 * Fs // 1024
        assert good(_create(L, [(0, lim, 0.0, 0)], Fs=Fs)) and _create(L, [(0, lim + 1, 0.0, 0)], Fs=Fs) == UNSUPPORTED, Fs
    assert good(_create(L, [(0, 0, 0.0, 0)])) and _create(L, [(0, -1, 0.0, 0)]) == BAD_ARG                       # doppler_millihz >= 0
    assert _create(L, [(-1, 20000, 0.0, 0)]) == BAD_ARG and _create(L, [(2, 20000, 0.0, 0)]) == BAD_ARG         # the path index
    assert good(_create(L, [(0, 20000, 0.0, 0)])) and good(_create(L, [(1, 20000, 0.0, 0)]))
    assert _create(L, [(0, 20000, 0.0, 0), (0, 20000, 1.0, 1)]) == BAD_ARG                                      # two fades on one path
    assert good(_create(L, [(0, 20000, 0.0, 0), (1, 20000, 0.0, 0)]))
    for k in (-1e-30, -1.0, float("nan"), float("inf"), float("-inf")):
        assert _create(L, [(0, 20000, k, 0)]) == BAD_ARG, k
    assert good(_create(L, [(0, 20000, 0.0, 0)])) and good(_create(L, [(0, 20000, 3.0e38, 0)]))
    assert _create(L, [], nfades=-1) == BAD_ARG and good(_create(L, [], nfades=0)) and good(_create(L, [], nfades=0, null=True))
    assert _create(L, [(0, 20000, 0.0, 0)], null=True) == BAD_ARG                                               # fades NULL with nfades > 0
    # a refused fade comes before an unsupported one, and the limits of pirip_hip_air_create_ex stand
    assert _create(L, [(0, 10 ** 9, 0.0, 0), (1, 5, -1.0, 0)]) == BAD_ARG
    assert _create(L, [(0, 5, 0.0, 0)], Fs=1) == BAD_ARG and _create(L, [(0, 5, 0.0, 0)], Fs=(1 << 24) + 1) == UNSUPPORTED
    # the table's entry point: host only
    import pirip_amd
    w, th = (C.c_int32 * 16)(), (C.c_uint32 * 16)()
    s, los = C.c_float(), C.c_float()
    f = pirip_amd.AirFade(0, 20000, 0.0, 0)
    args = (C.addressof(w), C.addressof(th), C.byref(s), C.byref(los))
    assert L.pirip_hip_air_fade_table(240000, 1, C.byref(f), *args) == 0
    assert L.pirip_hip_air_fade_table(240000, 1, None, *args) == BAD_ARG and L.pirip_hip_air_fade_table(240000, 1, C.byref(f), None, *args[1:]) == BAD_ARG
    assert L.pirip_hip_air_fade_table(240000, 1, C.byref(pirip_amd.AirFade(0, 234376, 0.0, 0)), *args) == UNSUPPORTED
    assert L.pirip_hip_air_fade_table(240000, 1, C.byref(pirip_amd.AirFade(0, 234375, 0.0, 0)), *args) == 0
    assert L.pirip_hip_air_fade_table(240000, 1, C.byref(pirip_amd.AirFade(0, 5, float("nan"), 0)), *args) == BAD_ARG


def test_fade_table_is_its_definition(built_lib):
    """pirip_hip_air_fade_table against the formula restated in Python: theta, scale and los exact, w within one unit (libm's cos may
    differ in the last place)"""
    for Fs, seed, fade in [(240000, 1, (0, 20.0, 0.0, 0)), (1 << 24, 79, (3, 16384.0, 1.0, 5)), (40000, 2 ** 63 + 5, (0, 0.007, 4.0, 2 ** 32 - 1)),
                           (240000, 1, (0, 234.375, 1.0e6, 9))]:
        w, th, s, los = faderef.table(Fs, seed, fade)
        w2, th2, s2, los2 = faderef.table_py(Fs, seed, fade)
        assert np.array_equal(th, th2) and s == s2 and los == los2, (Fs, fade)
        assert np.abs(w - w2).max() <= 1, (Fs, fade, w, w2)
        K = faderef.fade_of(fade)[2]
        assert abs(16 * s * s + los * los - 1.0) < 4e-7 and np.isclose(faderef.gamma((w, th, s, los)), np.sqrt(K / (K + 1)) + 4 / np.sqrt(K + 1))
        lim = 2 ** 32 * faderef.fade_of(fade)[1] / 1000.0 / Fs
        assert np.abs(w).max() <= lim + 1 and np.abs(w).max() <= 2 ** 22
        if fade[1] >= 1.0:                                            # one scatterer per sixteenth of the circle: both signs, spread out
            assert (w > 0).any() and (w < 0).any() and len(set(w.tolist())) == 16
    assert faderef.gamma(faderef.table(240000, 1, (0, 20.0, 0.0, 0))) == 4.0
    # Doppler 0: nothing moves
    w0, th0, _, _ = faderef.table(240000, 1, (0, 0.0, 0.0, 0))
    assert not w0.any() and np.array_equal(th0, faderef.table(240000, 1, (0, 20.0, 0.0, 0))[1])
    # two keys, two seeds: different tables; the path index does not count
    a, b, c = faderef.table(240000, 1, (0, 20.0, 0.0, 0)), faderef.table(240000, 1, (0, 20.0, 0.0, 1)), faderef.table(240000, 2, (0, 20.0, 0.0, 0))
    assert not np.array_equal(a[1], b[1]) and not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], c[1])
    import pirip_amd
    assert np.array_equal(pirip_amd.air_fade_table(240000, 1, (5, 20.0, 0.0, 0))[0], a[0])
    # the same (seed, key) at two values of Fs: the same draws, w scaled by the ratio (each rounded once)
    lo, hi = faderef.table(240000, 1, (0, 20.0, 1.0, 3)), faderef.table(480000, 1, (0, 20.0, 1.0, 3))
    assert np.array_equal(lo[1], hi[1]) and lo[2:] == hi[2:] and np.abs(lo[0] - 2 * hi[0]).max() <= 2


def test_model_on_a_case_worked_by_hand():
    """one path, Fs 64, three grid cells, 40 samples, on a table chosen so that the sums can be done by hand: scatterer 0 turns by a
    quarter per grid step (w = 2^26: 2 pi / 64 per sample), scatterer 1 stands at phase 0, and the other fourteen stand in seven pairs
    half a turn apart, which cancel. With s = 1/4 and los = 0: c_k = (1 + j^k) / 4."""
    w = np.zeros(16, dtype=np.int64)
    w[0] = 1 << 26
    theta = np.zeros(16, dtype=np.int64)
    for j in range(2, 16, 2):
        theta[j], theta[j + 1] = 12345 * j, (12345 * j + (1 << 31)) % (1 << 32)
    tab = (w, theta, 0.25, 0.0)
    print("table: w", w.tolist(), "theta", theta.tolist(), "s 0.25 los 0")
    c = faderef.grid(tab, np.arange(4))
    assert np.allclose(c, [0.5, 0.25 + 0.25j, 0.0, 0.25 - 0.25j], atol=1e-6)      # (the pairs' phases are cut to 24 bits: they cancel to 2^-23)
    g = faderef.gain(tab, np.arange(40))
    assert np.allclose(g[[0, 8, 16, 24, 32, 36]], [0.5, 0.375 + 0.125j, 0.25 + 0.25j, 0.125 + 0.125j, 0.0, 0.0625 - 0.0625j], atol=1e-6)
    # the grid is absolute: a start inside a cell continues the line, and the index counts modulo 2^32
    assert np.array_equal(faderef.gain(tab, 5 + np.arange(20)), g[5:25]) and np.allclose(faderef.gain(tab, 2 ** 32 + np.arange(40)), g, atol=1e-12)
    # through the model: a unit sample 3 late, gain 2, rotated by a quarter turn per sample (f = 16 at Fs = 64), at the receiver's index
    x = np.zeros((1, 40), dtype=np.complex128)
    x[0, 5], x[0, 21] = 1.0, 1j
    paths, fades = [(0, 0, 2.0, 3, 16)], [(0, 1.0, 0.0, 0)]
    y = faderef.signal(x, 64, paths, fades, 1, 0, 0, tabs={0: tab})
    assert np.isclose(y[8], 2.0 * (1j ** 8) * 1.0 * (0.375 + 0.125j)) and np.isclose(y[24], 2.0 * (1j ** 24) * 1j * (0.125 + 0.125j))
    assert np.count_nonzero(np.abs(y) > 1e-6) == 2
    # started at n0 = 16: the receiver's index 16 + 8 = 24 picks the gain, whatever the delay
    y = faderef.signal(x, 64, paths, fades, 1, 0, 16, tabs={0: tab})
    assert np.isclose(y[8], 2.0 * (1j ** 24) * (0.125 + 0.125j))
    # without a fade it is driftref's model, and the bound is driftref's
    assert np.array_equal(faderef.signal(x, 64, paths, [], 1, 0, 7), driftref.signal(x, 64, paths, 0, 7))
    assert faderef.bound(x, 64, paths, [], 1, 0) == driftref.bound(x, paths, 0)
    # the bound's arithmetic at K = 0: Gamma = 4, and 2 (272 / 4 + 16) + 8 sqrt 2 per fade
    faderef._TABLES[(64, 1, 1000, 0.0, 0)] = tab
    e = airref.E
    assert np.isclose(faderef.fade_terms(tab), 2 * (68 + 16) + 8 * np.sqrt(2))
    assert np.isclose(faderef.bound(x, 64, paths, fades, 1, 0), 13 * e * (2.0 * 4.0) + faderef.fade_terms(tab) * e * 2.0, rtol=1e-14)
    del faderef._TABLES[(64, 1, 1000, 0.0, 0)]


def _nu(tab, Fs):
    return tab[0].astype(np.float64) * Fs / 2.0 ** 32


@pytest.mark.parametrize("K", [0.0, 4.0])
def test_mean_power_of_the_model_is_one(built_lib, K):
    """|g|^2 = |los + s sum_j e^{j phi_j}|^2 = los^2 + 16 s^2 + s^2 sum_{i != j} e^{j (phi_i - phi_j)} + 2 los s Re sum_j e^{j phi_j}, and
    los^2 + 16 s^2 = 1. A cross term of the scatterers turns at nu_i - nu_j, and the mean of e^{j 2 pi d t} over a span T is sinc(d T) in
    modulus, at most 1 / (pi |d| T): the time average of |g|^2 is 1 within  sum_{i != j} s^2 / (pi |nu_i - nu_j| T),  the bound asserted
    here, with nu_j = w_j Fs / 2^32 from the table's own w. What it leaves aside is printed beside it and is small against it: for K > 0 the
    line of sight's cross terms, 2 los s sum_j 1 / (pi |nu_j| T); the mean over grid points 16 / Fs apart in place of the integral (a factor
    x / sin x with x = pi d 16 / Fs < 0.051, below 1.0005); the floats s and los (los^2 + 16 s^2 within 4e-7 of 1) and the phases cut to 24
    bits (4e-7 per term)."""
    Fs, T = 40000, 60.0
    tab = faderef.table(Fs, 1, (0, 20.0, K, 0))
    k = np.arange(int(T * Fs) // 16, dtype=np.int64)
    p = float(np.mean(np.abs(faderef.grid(tab, k)) ** 2))
    nu = _nu(tab, Fs)
    d = np.abs(nu[:, None] - nu[None, :])
    off = ~np.eye(16, dtype=bool)
    b = float((tab[2] ** 2 / (np.pi * d[off] * T)).sum())
    los_terms = float((2.0 * tab[3] * tab[2] / (np.pi * np.abs(nu) * T)).sum())
    print(f"K {K}: mean |g|^2 over {T:.0f} s = {p:.6f}; bound on its distance from 1 {b:.2e} (the line of sight's cross terms would add {los_terms:.2e}); "
          f"smallest |nu_i - nu_j| {d[off].min():.3f} Hz")
    assert d[off].min() > 0.05 and b < 0.05
    assert abs(p - 1.0) <= b


def _bessel_j0(x):
    """J0(x) = (1 / pi) int_0^pi cos(x sin t) dt, by the periodic trapezoid rule (exact to rounding for x << the number of points)"""
    t = (np.arange(4096) + 0.5) * (np.pi / 4096)
    return np.cos(np.asarray(x)[:, None] * np.sin(t)[None, :]).mean(axis=1)


def test_autocorrelation_of_the_scatter_part_follows_j0(built_lib):
    """Clarke's model: the scatter part h = s sum_j e^{j phi_j} has E h(t + tau) h*(t) = J0(2 pi f_d tau). Per key the time average over
    20 s at lags up to 1 / f_d is taken from the model's grid points (Fs 40000, 20 Hz, K = 0); 16 scatterers give every key its own curve,
    so only the ensemble is held to J0: the mean over 64 keys within 4 standard errors, the standard error from the 64 values."""
    Fs, fd, T, keys = 40000, 20.0, 20.0, 64
    npts = int(T * Fs) // 16
    lags = np.arange(0, int(Fs / fd) // 16 + 1, 5)
    tau = lags * 16.0 / Fs
    j0 = _bessel_j0(2.0 * np.pi * fd * tau)
    k = np.arange(npts, dtype=np.int64)
    R = np.zeros((keys, lags.size))
    for key in range(keys):
        tab = faderef.table(Fs, 1, (0, fd, 0.0, key))
        h = tab[2] * faderef.scatter(tab, k)
        R[key] = [float(np.mean(h[m:] * np.conj(h[:npts - m])).real) for m in lags]
    mean, se = R.mean(axis=0), R.std(axis=0, ddof=1) / np.sqrt(keys)
    print(f"largest |R - J0| of one key {np.abs(R - j0).max():.3f}, of the ensemble mean {np.abs(mean - j0).max():.4f}; "
          f"largest |mean - J0| / standard error {np.max(np.abs(mean - j0) / se):.2f}")
    assert (np.abs(mean - j0) <= 4.0 * se).all()


def _cases():
    for Fs in fs.FSS:
        for in_fmt in ("u8", "cf32"):
            x, paths, fades = fs.inputs(Fs, in_fmt)
            xw = airref.widen(x, fs.FMT[in_fmt])
            for n0 in fs.STARTS:
                for sigma in (None, fs.SIGMA):
                    yield Fs, in_fmt, xw, paths, fades, n0, sigma


def test_every_u8_case_stays_clear_of_the_quantisers_ties(built_lib):
    worst = 0.0
    for Fs, in_fmt, xw, paths, fades, n0, sigma in _cases():
        for r in range(fs.NRX):
            s = 0.0 if sigma is None else sigma[r]
            nz = airref.noise(fs.SEED, r, n0, fs.N, s)
            y = faderef.signal(xw, Fs, paths, fades, fs.SEED, r, n0) + nz
            b = faderef.bound(xw, Fs, paths, fades, fs.SEED, r, np.abs(nz)) if s else faderef.bound(xw, Fs, paths, fades, fs.SEED, r)
            _, v = airref.quantise_u8(y)
            share = float(airref.tie_window(v, b).mean())
            worst = max(worst, share)
            assert share <= 1e-3, (Fs, in_fmt, n0, r, s, share)
            assert np.abs(y).max() > 100 * np.max(b), "the test signal should not vanish in the bound"
    for Fs in (240000,):
        paths, fades = fs.cut_paths(Fs)
        x, _ = sh.inputs(Fs, "u8", n=fs.CUT_N, ntx=2, seed=60)
        xw = airref.widen(x, airref.U8)
        for r, s in enumerate(fs.CUT_SIGMA):
            nz = airref.noise(fs.CUT_SEED, r, fs.CUT_START, fs.CUT_N, s)
            y = faderef.signal(xw, Fs, paths, fades, fs.CUT_SEED, r, fs.CUT_START, age0=fs.CUT_AGE) + nz
            _, v = airref.quantise_u8(y)
            share = float(airref.tie_window(v, faderef.bound(xw, Fs, paths, fades, fs.CUT_SEED, r, np.abs(nz))).mean())
            worst = max(worst, share)
            assert share <= 1e-3, ("cut", r, share)
    print(f"largest share of components inside a tie window {worst:.2e}")


def test_shapes_reach_every_corner(built_lib):
    T = airref.TILE
    assert fs.N > 3 * T and fs.N % T and fs.N % 8 and sum(fs.CALLS) == fs.N
    s = fs.STARTS
    assert s[0] == 0 and s[1] & 15 == 15 and s[2] % 16 == 1 and (s[2] + T - 1) % 16 == 0 and s[0] % 16 == 0
    assert s[3] < 2 ** 32 < s[3] + fs.CALLS[0] and s[4] == 2 ** 31 + 3 and s[5] + fs.N == 2 ** 53 - 1
    for Fs in fs.FSS:
        paths, fades = fs.layout(Fs)
        e, lim = Fs // 2 - 1, fs.doppler_limit_hz(Fs)
        assert ms.edge(Fs) == e and round(lim * 1000) == 1000 * Fs // 1024
        faded = {f[0]: f for f in fades}
        assert len(faded) == len(fades) and all(0 <= i < len(paths) for i in faded)
        mine = lambda r: [(i, p) for i, p in enumerate(paths) if p[0] == r]
        # receiver 0: static without a fade, fading static, two fading rotated paths of one transmitter at delays 1 and 65, both edges
        r0 = mine(0)
        assert any(i not in faded and not p[3] and not p[4] for i, p in r0) and any(i in faded and not p[3] and not p[4] for i, p in r0)
        two = [(i, p) for i, p in r0 if i in faded and p[1] == 1]
        assert sorted(p[2] for _, p in two) == [1, 65] and sorted(p[3] for _, p in two) == [-e, e] and len({faded[i][3] for i, _ in two}) == 2
        # receiver 1: fading drifting paths of both signs inside the budget, one at the Doppler limit
        r1 = [(i, p) for i, p in mine(1) if p[4]]
        assert sorted(p[4] for _, p in r1) == [-300000, 300000] and all(i in faded for i, _ in r1) and any(faded[i][1] == lim for i, _ in r1)
        assert driftref.samples_left([(0, 0, 1.0) + p[2:] for _, p in r1], fs.MAX_SLIP, 0) >= fs.N
        assert all(p[2] >= 8 + (fs.MAX_SLIP if p[4] > 0 else 0) for _, p in r1)
        # receiver 2: the line of sight alone; receiver 3: Doppler 0 and the limit
        assert [faded[i][2] for i, _ in mine(2)] == [fs.K_LOS] and {faded[i][1] for i, _ in mine(3) if i in faded} == {0.0, lim}
        assert {faded[i][2] for i in faded} == {0.0, 1.0, fs.K_LOS}
        assert all(any(p[2] == 0 for _, p in mine(r)) for r in range(fs.NRX))      # no sample that is exactly 0, a tie of the quantiser
        assert 1.0 < faderef.gamma(faderef.table(Fs, fs.SEED, faded[mine(2)[0][0]])) < 1.005
        # at the limit a phase moves by up to 2 pi 16 / 1024 per grid step: w * 16 reaches 2^32 / 64
        wl = faderef.table(Fs, fs.SEED, faded[9])[0]
        assert 0.9 * 2 ** 26 < np.abs(wl).max() * 16 <= 2 ** 26 + 16
    # the tile's first output anywhere in a cell: the starts and the tiles behind them cover offsets 0, 1, 3, 12, 15
    assert {n0 % 16 for n0 in s} >= {0, 1, 3, 12, 15}
    # cutting: the longest delay above every cut but the last, rings that wrap, fades on drifting and static paths
    cp, cf = fs.cut_paths(240000)
    assert max(p[3] for p in cp) == 150 and driftref.rings(cp, 2, fs.CUT_SLIP) == [256, 128]
    assert {bool(driftref.ppb_of(cp[f[0]])) for f in cf} == {True, False} and driftref.samples_left(cp, fs.CUT_SLIP, fs.CUT_AGE) >= fs.CUT_N
    # a period of 2^32: static, unrotated
    assert all(not p[4] and not driftref.ppb_of(p) for p in fs.WRAP_PATHS)


@pytest.fixture(scope="module")
def fading_streams(built_lib, oracle):
    """the headline shape's noise-free test bits through the model: receiver 0 over a Rayleigh path of 20 Hz, receiver 1 over a Rician one
    (K = 4), quantised to u8; and |g| of either"""
    u8, bits = fs.demod_input(oracle)
    xw = airref.widen(u8[None], airref.U8)
    Fs = sigutil.CFG1["Fs"]
    idx = np.arange(xw.shape[1], dtype=np.int64)
    out = []
    for r in range(2):
        q, v = airref.quantise_u8(faderef.signal(xw, Fs, fs.DEMOD_PATHS, fs.DEMOD_FADES, fs.DEMOD_SEED, r, 0))
        assert ((v >= 0) & (v <= 255)).all()                       # Gamma times the amplitude stays inside the range
        out.append((q.astype(np.uint8), np.abs(faderef.gain(faderef.table(Fs, fs.DEMOD_SEED, fs.DEMOD_FADES[r]), idx))))
    return out, bits


@pytest.mark.parametrize("r", [0, 1], ids=["rayleigh", "rician"])
def test_oracle_demodulates_through_a_fading_path(oracle, fading_streams, r):
    """the reason for the feature: no bit error after the first frame in every frame whose smallest |g| exceeds 0.05, and at most a fifth
    of the frames left out"""
    streams, bits = fading_streams
    u8, gmag = streams[r]
    ro, N = fs.ds.clock_demod(oracle, u8)
    c = sigutil.CFG1
    frames, out, bad = fs.demod_check(ro, N + 2 * (c["Fs"] // c["Rs"]), bits, gmag)
    print(f"{'rayleigh' if r == 0 else 'rician'}: {frames} frames, {out} left out, frames with errors {bad}; |g| from {gmag.min():.3f} to {gmag.max():.3f}, "
          f"mean |g|^2 {np.mean(gmag ** 2):.3f}")
    assert frames >= 35 and out <= (frames - 1) / 5 and not bad
    assert gmag.max() / gmag.min() > 3.0                            # the level moved


def test_far_leg_of_the_loop_decodes_through_a_rician_path(built_lib, oracle):
    """tests/test_air_cpu.py's proof of the far leg with the far path Rician (K = 4, 5 Hz), either key of fadeshapes.LOOP_FADES: every
    frame of every channel without a bit error"""
    from test_air_cpu import decode_u8, loop_transmit_u8
    lp = ms.LOOP
    u8, rec, hb = loop_transmit_u8(oracle)
    p = sh.FAR
    xw = airref.widen(u8[None].astype(np.uint8), airref.U8)
    kb = rec.shape[2] - 1
    for f in fs.LOOP_FADES:
        y = faderef.receive(xw, lp["Fs"], [(0, 0, p["gain"], p["delay"], p["offset"])], [(0,) + f[1:]], sh.LOOP_SEED, 0, 0, sigma=sh.LOOP_SIGMA)
        q, _ = airref.quantise_u8(y)
        for c, good in enumerate(decode_u8(oracle, q, hb)):
            assert good.shape[0] == lp["nframes"], (f, c, good.shape[0])
            assert np.array_equal(good[:, :kb - 2], rec[c, :lp["nframes"], 1:kb - 1]), (f, c)
