"""The wave kernel's packed window powers and the ppm smoother's constant divide, as far as a CPU can check them.

1. The fine-timing sum in float32, in both orders of the four squares of a window start -- tone by tone (x0^2 + y0^2) + (x1^2 + y1^2),
   and packed (x0^2 + x1^2) + (y0^2 + y1^2) -- over the ORACLE's window sums of every frame of every stream the device test runs
   (tests/wpshapes.py). The two estimates differ by less than 5e-6 symbols, a tenth of DESIGN.md 5's 5e-5.
2. On the oracle alone: every such stream's norm_rx_timing keeps 5e-4 symbols away from +-0.25 and +-0.5 in every frame, so the device
   test can demand the exact nin sequence of every stream; the clean streams put floor(rx_timing) below, at and above zero and the
   drifting ones step nin in both directions.
3. x / 50 and x / 3 as the corrected product (fsk_device.hpp: div_rn_const) against the IEEE quotient for negative x: a strided
   sample of every float of the domain and both ends of every binade (tools/div_const_check.c runs all of them).

A fused multiply-add is stated as a float64 product and sum rounded to float32: exact products, and a sum that rounds twice in about one
case in 2^29 -- a disagreement of the divide check is therefore re-examined in exact rational arithmetic before it counts.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import wpshapes as wp
from demodrun import make_oracle

f32 = np.float32


class _Comp(C.Structure):
    _fields_ = [("real", C.c_float), ("imag", C.c_float)]


class _Recalled(C.Structure):
    _fields_ = [("hann_denominator_ndft", C.c_int), ("tc", C.c_float), ("est_space_rs", C.c_float), ("nin_threshold", C.c_float),
                ("nin_step_div", C.c_int), ("s16_scale", C.c_float), ("u8d_offset", C.c_float), ("u8d_scale", C.c_float),
                ("ndft_rule", C.c_int), ("sf_power", C.c_int)]


class _OracleFsk(C.Structure):
    """struct ORACLE_FSK (oracle/fsk_oracle.h) up to its test hook dbg_f_int, the last frame's window sums [M][(Nsym + 1) P]: the
    oracle has no getter for it. _window_sums checks the mirror against the fields that have one before it trusts the pointer."""
    _fields_ = [("rc", _Recalled), ("nin_step", C.c_int)] + \
               [(k, C.c_int) for k in ("Ndft", "Fs", "N", "Rs", "Ts", "Nmem", "P", "Nsym", "Nbits", "f1_tx", "tone_spacing", "mode")] + \
               [("tc", C.c_float), ("est_min", C.c_int), ("est_max", C.c_int), ("est_space", C.c_int), ("hann_table", C.c_void_p),
                ("Sf", C.c_void_p), ("phi_c", _Comp * 4), ("f_dc", C.c_void_p), ("fft_cfg", C.c_void_p), ("norm_rx_timing", C.c_float),
                ("tx_phase_c", _Comp), ("EbNodB", C.c_float), ("f_est", C.c_float * 4), ("f2_est", C.c_float * 4), ("freq_est_type", C.c_int)] + \
               [(k, C.c_float) for k in ("ppm", "SNRest", "v_est", "rx_sig_pow", "rx_nse_pow")] + \
               [("nin", C.c_int), ("burst_mode", C.c_int), ("lock_nin", C.c_int), ("stats", C.c_float * 8), ("dbg_f_int", C.POINTER(C.c_float))]


def _window_sums(o, c):
    s = _OracleFsk.from_address(o.h)
    o.l.oracle_fsk_get_Sf.restype = C.c_void_p
    o.l.oracle_fsk_get_Sf.argtypes = [C.c_void_p]
    assert (s.Fs, s.Rs, s.P, s.Nsym, s.Ts, s.est_min, s.est_max) == (c["Fs"], c["Rs"], c["P"], wp.NSYM, c["Fs"] // c["Rs"], c["est_min"], c["est_max"])
    assert s.Sf == o.l.oracle_fsk_get_Sf(o.h) and s.nin == o.nin()
    nint = (wp.NSYM + 1) * c["P"]
    return np.ctypeslib.as_array(s.dbg_f_int, shape=(c["M"], nint, 2)).copy()


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def timing_both_orders(fi, P):
    """norm_rx_timing of one frame from its window sums fi [M][(Nsym + 1) P][re, im], the way the wave kernel sums (per symbol the P
    window starts in order onto one phasor pair, then the symbols' pairs turned by the recursion's gain and added), with |.|^2 summed
    over the tones (a) tone by tone, (b) packed. Returns (a, b) in symbols."""
    M = fi.shape[0]
    x, y = fi[..., 0].astype(f32), fi[..., 1].astype(f32)
    a = _fma(x[0], x[0], y[0] * y[0])
    sx, sy = x[0] * x[0], y[0] * y[0]
    for m in range(1, M):
        a = a + _fma(x[m], x[m], y[m] * y[m])
        sx, sy = _fma(x[m], x[m], sx), _fma(y[m], y[m], sy)
    b = sx + sy
    q = np.arange(P)
    tpx, tpy = np.cos(2 * np.pi * q / P).astype(f32), np.sin(2 * np.pi * q / P).astype(f32)
    g = np.exp(2j * np.pi * np.arange(wp.NSYM + 1))         # the recursion's gain at a symbol's first window start: 1 up to its drift
    gx, gy = g.real.astype(f32), g.imag.astype(f32)
    out = []
    for ft in (a, b):
        ft = ft.reshape(wp.NSYM + 1, P)
        pr = np.zeros(wp.NSYM + 1, f32); pi = np.zeros(wp.NSYM + 1, f32)
        for k in range(P):
            pr, pi = _fma(ft[:, k], np.broadcast_to(tpx[k], pr.shape), pr), _fma(ft[:, k], np.broadcast_to(tpy[k], pi.shape), pi)
        tcr = np.sum(pr * gx - pi * gy, dtype=f32); tci = np.sum(pr * gy + pi * gx, dtype=f32)
        out.append(f32(np.arctan2(tci, tcr)) * f32(0.15915494309189535))
    return out


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    """per instance and case: for every stream the oracle's stats rows and the two float32 timing estimates of every frame"""
    runs = {}
    for name, c in wp.PACKED.items():
        for case, make in wp.CASES.items():
            host = make(oracle, c)
            per_stream = []
            for s in range(host.shape[0]):
                o = make_oracle(oracle, c)
                pos, stats, ab = 0, [], []
                while pos + o.nin() <= host.shape[1]:
                    r = o.demod(host[s, pos:pos + o.nin()], c["fmt"], want_filt=False)
                    assert r["nframes"] == 1
                    pos += r["consumed"]
                    stats.append(r["stats"][0]); ab.append(timing_both_orders(_window_sums(o, c), c["P"]))
                per_stream.append((np.array(stats), np.array(ab, dtype=np.float64)))
            runs[name, case] = per_stream
    return runs


def test_streams_keep_clear_of_the_nin_thresholds_and_the_wrap(oracle_runs):
    for (name, case), per_stream in oracle_runs.items():
        assert len(per_stream) == 6
        for s, (st, _) in enumerate(per_stream):
            t = np.abs(st[:, 4].astype(np.float64))
            assert len(t) >= (wp.PPM_FRAMES if case == "drifting" else wp.CLEAN_FRAMES), (name, case, s, len(t))
            assert (np.abs(t - 0.25) >= wp.TIMING_MARGIN).all() and (0.5 - t >= wp.TIMING_MARGIN).all(), (name, case, s, st[:, 4])


def test_inputs_reach_both_select_branches_and_step_nin_both_ways(oracle_runs):
    for name, c in wp.PACKED.items():
        N, Q = c["Fs"] // c["Rs"] * wp.NSYM, c["Fs"] // c["Rs"] // 4
        low = np.concatenate([np.floor(st[2:, 4] * c["P"]) for st, _ in oracle_runs[name, "clean"]])
        assert (low < 0).any() and (low == 0).any() and (low > 0).any(), sorted(set(low.tolist()))
        nin = [st[:, 6] for st, _ in oracle_runs[name, "drifting"]]
        assert any((n == N + Q).any() for n in nin) and any((n == N - Q).any() for n in nin), [sorted(set(n.tolist())) for n in nin]
        # (the ppm smoother's dividend has both signs: timing falls from frame to frame in some streams and rises in others)
        d = np.concatenate([np.diff(st[:, 4]) for st, _ in oracle_runs[name, "drifting"]])
        assert (d < 0).sum() >= 20 and (d > 0).sum() >= 20


def test_the_two_summation_orders_agree_to_5e_6_symbols(oracle_runs):
    worst = 0.0
    for (name, case), per_stream in oracle_runs.items():
        for s, (st, ab) in enumerate(per_stream):
            d = np.abs(ab[:, 0] - ab[:, 1])
            worst = max(worst, float(d.max()))
            assert (d < 5e-6).all(), (name, case, s, d.max())
            if case != "noisy":
                # (and the statement is the device's sum: within DESIGN.md 5's bound of the oracle's own estimate)
                assert (np.abs(ab[:, 0] - st[:, 4]) < 5e-5).all(), (name, case, s, np.abs(ab[:, 0] - st[:, 4]).max())
    print(f"largest difference between the two orders: {worst:.3e} symbols")


def _div3op(x, c):
    c = f32(c); rc = f32(1.0) / c
    q = x * rc
    r = (-(q.astype(np.float64)) * np.float64(c) + x.astype(np.float64)).astype(f32)
    return (r.astype(np.float64) * np.float64(rc) + q.astype(np.float64)).astype(f32)


def _div3op_exact(x, c):
    """one value in exact rational arithmetic, every operation rounded once to float32"""
    def rn(fr):
        # round a Fraction to float32: through float64 only where that is exact enough to decide (else nudge by the remainder's sign)
        d = float(fr)
        lo = f32(d)
        if Fraction(float(lo)) == fr:
            return lo
        cands = sorted({f32(np.nextafter(lo, f32(-np.inf))), lo, f32(np.nextafter(lo, f32(np.inf)))}, key=float)
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - fr), int(v.view(np.uint32)) & 1))
        return best
    X, Cc = Fraction(float(x)), Fraction(c)
    rc = Fraction(float(f32(1.0) / f32(c)))
    q = rn(X * rc)
    r = rn(-Fraction(float(q)) * Cc + X)
    return rn(Fraction(float(r)) * rc + Fraction(float(q)))


@pytest.mark.parametrize("c, first", [(50, 0x81000000), (3, 0x80000001)])
def test_corrected_product_is_the_quotient_for_negative_arguments(c, first):
    """c = 50: x <= -2^-125; c = 3: every finite x < 0. (-0 is in neither domain: the corrected product gives +0.)"""
    bits = np.arange(first, 0xff7fffff, 1021, dtype=np.uint64)
    e = np.arange(first >> 23, 0x1ff, dtype=np.uint64) << np.uint64(23)
    edges = np.concatenate([e + np.uint64(m) for m in (0, 1, 2, 0x7ffffe, 0x7fffff)])
    edges = edges[(edges >= first) & (edges <= 0xff7fffff)]
    x = np.concatenate([bits, edges, [first, 0xff7fffff]]).astype(np.uint32).view(f32)
    assert (x < 0).all() and np.isfinite(x).all()
    with np.errstate(under="ignore"):
        want, got = x / f32(c), _div3op(x, c)
    bad = np.flatnonzero(want.view(np.uint32) != got.view(np.uint32))
    assert len(bad) < 8, (len(bad), x[bad][:8])                 # (double rounding of the float64 statement: re-examined exactly)
    for i in bad:
        assert _div3op_exact(x[i], c).view(np.uint32) == want[i].view(np.uint32), (x[i], want[i])
    # the one negative-side exception, stated: -0 / c is -0, the corrected product +0
    z = np.array([-0.0], dtype=f32)
    assert _div3op(z, c).view(np.uint32)[0] == 0 and (z / f32(c)).view(np.uint32)[0] == 0x80000000
