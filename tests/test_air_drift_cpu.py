"""The channel's drifting paths (include/pirip_hip.h section O, drift) without a GPU: the symbols, the binding and the
CLI option are there and every limit answers before a device is looked for; the interpolator's table is its definition; the model's
integers are Python's; the model on a case worked by hand; the inputs of tests/test_air_drift.py stay clear of the quantiser's ties and
reach what they claim; and the reason for the feature: the oracle demodulator tracks a clock 300 ppm off either way through the model."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import airref
import driftref
import driftshapes as ds
import muxshapes as ms

DRIFT_SYMBOLS = ("pirip_hip_air_create_ex", "pirip_hip_air_interp_table", "pirip_hip_air_get_drift", "pirip_hip_air_reset_drift")
BAD_ARG, UNSUPPORTED = -1, -6
Q = driftref.Q


def test_symbols_binding_cli_and_abi(built_lib):
    import pirip_amd
    out = subprocess.run(["nm", "-D", "--defined-only", pirip_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    hdr = open(os.path.join(ms.ROOT, "include", "pirip_hip.h")).read()
    for n in DRIFT_SYMBOLS:
        assert n in exported and hasattr(built_lib, n) and n + "(" in hdr, n
    assert "pirip_air_path_ex" in hdr and "#define PIRIP_HIP_ABI_VERSION 2" in " ".join(hdr.split())
    abi = C.c_int(0)
    assert built_lib.pirip_hip_abi(C.byref(abi), None, None) == 0 and abi.value == 2
    assert [f[0] for f in pirip_amd.AirPathEx._fields_] == ["rx", "tx", "delay", "offset_hz", "gain", "clock_ppb"]
    assert C.sizeof(pirip_amd.AirPathEx) == 24 and C.sizeof(pirip_amd.AirPath) == 20
    sig = inspect.signature(pirip_amd.HipAir)
    assert sig.parameters["max_slip"].default == 0
    assert inspect.signature(pirip_amd.HipAir.reset).parameters["age"].default == 0
    assert callable(pirip_amd.HipAir.drift)
    tool = os.path.join(ms.BIN, "air_channels")
    usage = subprocess.run([tool, "--help"], capture_output=True, text=True).stderr
    assert "--max-slip" in usage and "offset[,ppb]" in usage
    # the ppb field is an integer, and --max-slip is not negative: refused as arguments, before any file or device
    assert subprocess.run([tool, "--fs", "240000", "--path", "0,0,1.0,20,0,1.5", "a", "--", "b"], capture_output=True).returncode == 1
    assert subprocess.run([tool, "--fs", "240000", "--max-slip", "-1", "a", "--", "b"], capture_output=True).returncode == 1


def _create(L, paths, max_slip, Fs=240000, ntx=1, nrx=1):
    import pirip_amd
    arr = (pirip_amd.AirPathEx * max(len(paths), 1))()
    for i, (rx, tx, gain, delay, off, q) in enumerate(paths):
        arr[i] = pirip_amd.AirPathEx(rx, tx, delay, off, gain, q)
    h = C.c_void_p()
    rc = L.pirip_hip_air_create_ex(Fs, 1, 1, ntx, nrx, len(paths), C.addressof(arr), None, 1, max_slip, -1, C.byref(h))
    if rc == 0:
        L.pirip_hip_air_destroy(h)
    return rc


def test_every_limit_answers_before_a_device_is_looked_for(built_lib):
    """both sides of every PIRIP_ERR_BAD_ARG / PIRIP_ERR_UNSUPPORTED of the definition; the good side gets as far as the device (a handle,
    or PIRIP_ERR_NO_DEVICE here)"""
    L = built_lib
    good = lambda rc: rc not in (BAD_ARG, UNSUPPORTED)
    P = lambda d, q: [(0, 0, 1.0, d, 0, q)]
    top = 1 << 20
    assert _create(L, P(0, 0), -1) == BAD_ARG and good(_create(L, P(0, 0), 0)) and good(_create(L, P(0, 0), 7))     # max_slip < 0; no drift: any
    assert _create(L, P(100, 5), 0) == BAD_ARG and _create(L, P(100, -5), 0) == BAD_ARG and good(_create(L, P(100, 5), 1))   # drift wants max_slip >= 1
    assert _create(L, P(7, -1), 1) == BAD_ARG and good(_create(L, P(8, -1), 1))                                   # d >= 8
    assert _create(L, P(8 + 9, 1), 10) == BAD_ARG and good(_create(L, P(8 + 10, 1), 10)) and good(_create(L, P(8, -1), 10))    # ... + max_slip for q > 0
    assert _create(L, P(top - 7 + 1, 1), 1) == UNSUPPORTED and good(_create(L, P(top - 7, 1), 1))                 # d + 7 <= 2^20
    assert _create(L, P(top - 7 - 100 + 1, -1), 100) == UNSUPPORTED and good(_create(L, P(top - 7 - 100, -1), 100))   # ... + max_slip for q < 0
    assert good(_create(L, P(top - 7, 1), top - 15)) and _create(L, P(8, -1), top - 14) == UNSUPPORTED and good(_create(L, P(8, -1), top - 15))
    assert _create(L, P(100, 10 ** 6 + 1), 5) == UNSUPPORTED and _create(L, P(100, -10 ** 6 - 1), 5) == UNSUPPORTED
    assert good(_create(L, P(100, 10 ** 6), 5)) and good(_create(L, P(100, -10 ** 6), 5))
    # the limits of pirip_hip_air_create stand
    assert _create(L, P(-1, 0), 0) == BAD_ARG and _create(L, P(top + 1, 0), 0) == UNSUPPORTED and good(_create(L, P(top, 0), 0))
    assert _create(L, [(0, 0, float("nan"), 100, 0, 5)], 5) == BAD_ARG and _create(L, [(1, 0, 1.0, 100, 0, 5)], 5) == BAD_ARG
    assert L.pirip_hip_air_create_ex(240000, 1, 1, 1, 1, 1, None, None, 1, 0, -1, C.byref(C.c_void_p())) == BAD_ARG
    assert L.pirip_hip_air_create_ex(240000, 1, 1, 1, 1, 0, None, None, 1, 0, -1, None) == BAD_ARG
    # the other entry points on no handle
    assert L.pirip_hip_air_get_drift(None, None, None) == BAD_ARG and L.pirip_hip_air_reset_drift(None, 0, 0, None) == BAD_ARG
    assert L.pirip_hip_air_interp_table(None, None, None) == BAD_ARG


def test_table_is_its_definition(built_lib):
    T = driftref.table()
    assert T.dtype == np.float32 and T.shape == (1024, 16)
    unit = np.zeros(16, dtype=np.float32)
    unit[7] = 1.0
    assert np.array_equal(T[0], unit) and not np.signbit(T[0]).any()                      # phase 0: the exact unit impulse
    ref = driftref.table_f64()
    assert np.abs(T.astype(np.float64) - ref).max() <= 2.0 ** -24
    assert np.abs(T.astype(np.float64).sum(axis=1) - 1.0).max() <= 16 * 2.0 ** -24
    lam = driftref.lam()
    print(f"Lambda = {lam:.6f}")
    assert 1.0 < lam < 2.2
    # pirip_hip_air_interp_table with the optional pointers NULL gives the same floats
    t2 = np.zeros((1024, 16), dtype=np.float32)
    assert built_lib.pirip_hip_air_interp_table(t2.ctypes.data, None, None) == 0 and np.array_equal(t2, T)


@pytest.mark.parametrize("q", [300000, -300000, 10 ** 6, 37])
def test_model_reproduces_unit_tones_within_half_a_u8_level(built_lib, q):
    """x[j] = e^{j 2 pi f j} read at n - d + m q / Q: the model on the library's table against the tone itself, |f| / Fs in {1/16, 1/8,
    1/4, 3/8}; the clock ages sweep every phase (37 ppb needs ages up to 2.7 10^7 for that)"""
    n, d = 4096, 64
    ages = [0, 3 * 10 ** 6 + 1, 13 * 10 ** 6 + 7, 26 * 10 ** 6] if q == 37 else [0, 1234]
    worst = 0.0
    j = np.arange(n, dtype=np.int64)
    for f in (1 / 16, -1 / 8, 1 / 4, -3 / 8, 3 / 8):
        x = np.exp(2j * np.pi * f * j)
        for age in ages:
            S, rho, _ = driftref.slip(age + j, q)
            pos = (j - d + S) + rho / Q                            # the read position, n - d + m q / Q
            got = driftref.interpolate(x, d, q, age)
            live = j - d + S - 7 >= 0                              # every tap on the tone
            worst = max(worst, float(np.abs(got - np.exp(2j * np.pi * f * pos))[live].max()))
    print(f"q {q}: largest error on a unit tone {worst:.3e}")
    assert worst <= 1 / 255


@pytest.mark.parametrize("q", [1, -1, 999999937, -999999937, 10 ** 6, -10 ** 6])
@pytest.mark.parametrize("max_slip", [1, ds.SLIP_LARGE])
def test_slip_arithmetic_is_pythons(q, max_slip):
    """S, rho and phi of the model's int64 arithmetic against Python's integers at the budget's last accepted clock age and the first
    refused one, and the budget itself: |S| <= max_slip exactly up to the last age"""
    last = driftref.last_age(max_slip, q)
    for m in (0, 1, last - 1, last, last + 1):
        S, rho, phi = (int(v[0]) for v in driftref.slip(np.array([m], dtype=np.int64), q))
        mq = m * q
        assert S == mq // Q and rho == mq - Q * (mq // Q) and 0 <= rho < Q and phi == (1024 * rho) // Q and 0 <= phi < 1024, (q, m)
        assert abs(mq) < 2 ** 51
        assert (abs(S) <= max_slip) == (m <= last), (q, max_slip, m, S)
    # the two checks as the header states them, without the division
    if q > 0:
        assert last * q < (max_slip + 1) * Q <= (last + 1) * q
    else:
        assert last * -q <= max_slip * Q < (last + 1) * -q
    assert driftref.samples_left([(0, 0, 1.0, 100, 0, q)], max_slip, last) == 1 and driftref.samples_left([(0, 0, 1.0, 100, 0, q)], max_slip, last + 1) == 0
    assert driftref.samples_left([(0, 0, 1.0, 100, 0, 0)], max_slip, 5) is None


def test_model_on_a_case_worked_by_hand(built_lib):
    """three samples, one phase: at clock age 500 a clock 10^6 ppb fast has slipped 0.5 samples -- S = 0, rho = Q / 2, phase 512 -- and a
    slow one -0.5: S = -1, the same phase"""
    T = driftref.table().astype(np.float64)
    assert driftref.slip(500, 10 ** 6) == (0, Q // 2, 512) and driftref.slip(500, -10 ** 6) == (-1, Q // 2, 512)
    x = np.zeros((1, 20), dtype=np.complex128)
    x[0, 8:11] = [1.0, 2j, -3.0]
    # output 17 at age0 = 483, delay 8, fast: i = 17 - 8 + 0 = 9, tap k reads x[2 + k]: taps 6, 7, 8 meet the three samples
    y = driftref.signal(x, 8, [(0, 0, 2.0, 8, 0, 10 ** 6)], 0, 0, age0=483)
    assert y[17] == 2.0 * (T[512, 6] * 1.0 + T[512, 7] * 2j + T[512, 8] * -3.0)
    # slow, delay 8: i = 17 - 8 - 1 = 8, tap k reads x[1 + k]: taps 7, 8, 9
    y = driftref.signal(x, 8, [(0, 0, 1.0, 8, 0, -10 ** 6)], 0, 0, age0=483)
    assert y[17] == T[512, 7] * 1.0 + T[512, 8] * 2j + T[512, 9] * -3.0
    # rotated by the receiver's index, e^{j 2 pi 2 n / 8} = j^n at n = 6 + 17
    y = driftref.signal(x, 8, [(0, 0, 1.0, 8, 2, -10 ** 6)], 0, 6, age0=483)
    assert np.isclose(y[17], (1j ** 23) * (T[512, 7] * 1.0 + T[512, 8] * 2j + T[512, 9] * -3.0))
    # q = 0 is airref's path, and a path of five elements is one of q = 0
    p5, p6 = [(0, 0, 0.5, 3, 1)], [(0, 0, 0.5, 3, 1, 0)]
    assert np.array_equal(driftref.signal(x, 8, p6, 0, 6), airref.signal(x, 8, p5, 0, 6)) and np.array_equal(driftref.signal(x, 8, p5, 0, 6), airref.signal(x, 8, p5, 0, 6))
    # the bound: airref's with Lambda on the drifting path and its sixteen roundings
    e, L = airref.E, driftref.lam()
    paths = [(0, 0, 0.5, 8, 0, 0), (0, 0, -0.25, 8, 7, 5)]
    A = 0.5 * 3.0 + 0.25 * 3.0 * L
    assert np.isclose(driftref.bound(x, paths, 0), 14 * e * A + 16 * e * L * 0.25 * 3.0, rtol=1e-14)
    assert driftref.bound(x, paths[:1], 0) == airref.bound(x, [paths[0][:5]], 0) and driftref.bound(x, paths, 1) == 0.0
    assert driftref.rings([(0, 0, 1.0, 57, 0, 1), (0, 1, 1.0, 50, 0, -1), (0, 2, 1.0, 64, 0, 0), (0, 3, 1.0, 58, 0, 5)], 4, 8) == [64, 128, 64, 128]


def _cases():
    for Fs in ds.FSS:
        for in_fmt in ("u8", "cf32"):
            for max_slip, age, n0 in ds.RUNS:
                x, paths = ds.inputs(Fs, in_fmt, max_slip)
                xw = airref.widen(x, ds.FMT[in_fmt])
                for sigma in (None, ds.SIGMA):
                    yield Fs, in_fmt, xw, paths, max_slip, age, n0, sigma


def test_every_u8_case_stays_clear_of_the_quantisers_ties(built_lib):
    worst = 0.0
    for Fs, in_fmt, xw, paths, max_slip, age, n0, sigma in _cases():
        for r in range(ds.NRX):
            s = 0.0 if sigma is None else sigma[r]
            nz = airref.noise(ds.SEED, r, n0, ds.N, s)
            y = driftref.signal(xw, Fs, paths, r, n0, age0=age) + nz
            b = driftref.bound(xw, paths, r, np.abs(nz)) if s else driftref.bound(xw, paths, r)
            _, v = airref.quantise_u8(y)
            share = float(airref.tie_window(v, b).mean())
            worst = max(worst, share)
            assert share <= 1e-3, (Fs, in_fmt, max_slip, age, r, s, share)
            assert np.abs(y).max() > 100 * np.max(b), "the test signal should not vanish in the bound"
    print(f"largest share of components inside a tie window {worst:.2e}")


def test_shapes_reach_every_corner():
    T = airref.TILE
    assert ds.N > 3 * T and ds.N % T and ds.N % 8 and sum(ds.CALLS) == ds.N and ds.SLIP_LARGE == 2 ** 20 - 4096 - 7
    for max_slip, age, n0 in ds.RUNS:
        for Fs in ds.FSS:
            lay = ds.layout(Fs, max_slip)
            qs = {q for *_, q in lay}
            assert qs == {0, 1, -1, 300000, -300000, 10 ** 6, -10 ** 6}
            for r in range(ds.NRX):                                # every receiver mixes static and drifting paths of one transmitter
                mine = [p for p in lay if p[0] == r]
                assert any(p[4] == 0 and any(o[4] != 0 and o[1] == p[1] for o in mine) for p in mine), r
            assert all(d >= 8 + (max_slip if q > 0 else 0) for _, _, d, _, q in lay if q)
            assert all(d + 7 + (max_slip if q < 0 else 0) <= 2 ** 20 for _, _, d, _, q in lay if q)
            assert min(d for _, _, d, _, q in lay if q < 0) == 8 and min(d for _, _, d, _, q in lay if q > 0) == 8 + max_slip
            assert T + 1 in {d for _, _, d, _, q in lay if q}
            if max_slip == ds.SLIP_SMALL:
                assert {63, 64, 65} <= {d for _, _, d, _, q in lay if q}
            # the whole run stays inside the budget, and for the large one its last sample sits on it
            left = driftref.samples_left([(0, 0, 1.0) + p[2:] for p in lay], max_slip, age)
            assert left >= ds.N
            if max_slip == ds.SLIP_LARGE:
                assert left == ds.N
                for q in (10 ** 6, -10 ** 6):
                    assert abs(int(driftref.slip(age + ds.N - 1, q)[0])) == max_slip
    # where S steps for +-300000 ppb: inside a tile, on a tile's first sample, on the second call's first sample
    def steps(age, q):
        S = driftref.slip(age + np.arange(ds.N, dtype=np.int64), q)[0]
        return (np.flatnonzero(np.diff(S)) + 1).tolist()
    for q in (300000, -300000):
        assert steps(0, q) == [1, 3334][q > 0:] and 3334 % T
        assert steps(1286, q)[-2 if q > 0 else -2] == T or T in steps(1286, q)
        assert ds.CALLS[0] in steps(2167, q) and any(s % T and s < T for s in steps(2167, q))
    assert all(len([s for s in steps(a, 10 ** 6) if t * T < s < (t + 1) * T]) >= 1 for a in (0, 1286, 2167) for t in range(3))
    # cutting: S steps inside the run for every offset but +-1, the run stays inside its budget, both rings wrap under a lag
    cp = ds.cut_paths(240000)
    assert driftref.rings(cp, 2, ds.CUT_SLIP) == [256, 128] and ds.CUT_N > 256
    assert driftref.samples_left(cp, ds.CUT_SLIP, ds.CUT_AGE) >= ds.CUT_N
    for p in cp:
        q = driftref.ppb_of(p)
        S = driftref.slip(ds.CUT_AGE + np.arange(ds.CUT_N, dtype=np.int64), q)[0] if q else np.zeros(1)
        assert (len(np.unique(S)) > 1) == (abs(q) > 1), q
    assert all(d >= 8 + (ds.CUT_SLIP if q > 0 else 0) for _, _, _, d, _, q in cp if q)
    # the loop: far paths on two clocks, inside the budget for the whole run
    assert all(p[3] >= 8 + ds.LOOP_SLIP for p in ds.LOOP_PATHS if driftref.ppb_of(p) > 0)
    assert {driftref.ppb_of(p) for p in ds.LOOP_PATHS} == {0, ds.LOOP_PPB, -ds.LOOP_PPB}


@pytest.fixture(scope="module")
def clock_streams(built_lib, oracle):
    """the headline shape's test bits through the model, one path 300 ppm fast and one 300 ppm slow, quantised to u8"""
    u8, bits = ds.clock_input(oracle)
    xw = airref.widen(u8[None], airref.U8)
    paths = ds.clock_paths()
    assert driftref.samples_left(paths, ds.CLOCK_SLIP, 0) >= xw.shape[1]
    out = []
    for r in range(2):
        q, _ = airref.quantise_u8(driftref.signal(xw, 240000, paths, r, 0))
        out.append(q.astype(np.uint8))
    return out, bits


@pytest.mark.parametrize("r", [0, 1], ids=["fast", "slow"])
def test_oracle_tracks_a_clock_300_ppm_off_through_the_model(oracle, clock_streams, r):
    """the reason for the feature: no bit error after the first frame, and nin moves -- at least two short frames on the fast clock, two
    long ones on the slow one (tests/blockshapes.py's clock_counts_ok on the headline shape)"""
    streams, bits = clock_streams
    ro, N = ds.clock_demod(oracle, streams[r])
    nin = ro["stats"][:, 6]
    short, long_ = int((nin < N).sum()), int((nin > N).sum())
    res = oracle.put_test_bits(ro["bits"][1:].reshape(-1))
    print(f"{'fast' if r == 0 else 'slow'}: {ro['nframes']} frames, {short} short, {long_} long, {res['bits']} test bits, {res['errors']} errors")
    assert ro["nframes"] >= 35 and res["bits"] > 1500 and res["errors"] == 0
    assert (short if r == 0 else long_) >= 2


@pytest.mark.parametrize("ppb", [ds.LOOP_PPB, -ds.LOOP_PPB], ids=["fast", "slow"])
def test_far_leg_of_the_loop_decodes_on_two_clocks(built_lib, oracle, ppb):
    """tests/test_air_cpu.py's proof of the far leg with the leg's clock offset: the loop's transmit IQ through the model (gain, delay and
    offset of airshapes.FAR, the loop's sigma), quantised, then through the reference chain -- every frame of every channel without a
    bit error. The leaks stay static: tests/test_air_cpu.py proves them."""
    import airshapes as sh
    from test_air_cpu import decode_u8, loop_transmit_u8
    lp = ms.LOOP
    u8, rec, hb = loop_transmit_u8(oracle)
    p = sh.FAR
    xw = airref.widen(u8[None].astype(np.uint8), airref.U8)
    assert driftref.samples_left([(0, 0, 1.0, p["delay"], 0, ppb)], ds.LOOP_SLIP, 0) >= xw.shape[1]
    y = driftref.receive(xw, lp["Fs"], [(0, 0, p["gain"], p["delay"], p["offset"], ppb)], 0, 0, sigma=sh.LOOP_SIGMA, seed=sh.LOOP_SEED)
    q, _ = airref.quantise_u8(y)
    kb = rec.shape[2] - 1
    for c, good in enumerate(decode_u8(oracle, q, hb)):
        assert good.shape[0] == lp["nframes"], (ppb, c, good.shape[0])
        assert np.array_equal(good[:, :kb - 2], rec[c, :lp["nframes"], 1:kb - 1]), (ppb, c)
