"""include/pirip_hip.h section O: the channel (pirip_hip_air_*, pirip_amd.HipAir) and the CLI air_channels.

Contract 1: every complex-float component within airref.bound -- (K_r + 12) 2^-24 A_r, with noise plus txref.NOISE_REL_BOUND |sigma w| +
2^-24 (A_r + |sigma w|), derived in DESIGN.md 4.15 from the arithmetic -- of the float64 statement (tests/airref.py) on the same inputs,
gains and sigma; every u8 byte within one level of the quantised float64 value, and different from it only where the float64 argument
lies within 127.5 bound + 2^-16 of a tie. Contract 2, bit for bit: any cutting of the input into calls equals one shot, n0 equals
n0 + k Fs without noise, a receiver does not depend on the others, a sample-aligned row equals a 16-byte-aligned one, the noise is
HipTx.modulate's. Contract 3: terminal and repeater find each other over the shared medium, and each filters what it hears of itself.
tests/test_air_cpu.py shows on the model alone that the inputs used here reach what they claim."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import airref
import airshapes as sh
import muxshapes as ms
import txref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
BAD_ARG, UNSUPPORTED = -1, -6


def _fmt(name):
    import pirip_amd
    return pirip_amd.IN_CF32 if name == "cf32" else pirip_amd.IN_CU8_CSDR


def _run(air, x, calls, pad=0):
    """x: uint8 [ntx, n, 2] or complex64 [ntx, n], pushed in calls of the given lengths -> uint8 [nrx, n * bytes per output sample] as
    stored. Every call has rows of its own, 16-byte aligned with strides that are multiples of 16 (pad 0) or moved off by one sample, the
    strides too (pad 1). Every row lies between canary bytes."""
    import torch
    ntx, n = x.shape[0], x.shape[1]
    bsi, bso = air.in_bytes_per_sample, air.out_bytes_per_sample
    raw = np.ascontiguousarray(x).view(np.uint8).reshape(ntx, n * bsi)
    assert sum(calls) == n
    keep, at = [], 0
    for c in calls:
        in_stride = (c * bsi + 15) // 16 * 16 + 16 + (bsi if pad else 0)
        buf = np.full(ntx * in_stride + 64, 0x5A, dtype=np.uint8)
        for t in range(ntx):
            buf[pad * bsi + t * in_stride: pad * bsi + t * in_stride + c * bsi] = raw[t, at * bsi:(at + c) * bsi]
        d_in = torch.from_numpy(buf).cuda()
        out_stride = (c * bso + 32 + 15) // 16 * 16 + (bso if pad else 0)
        d_out = torch.full((air.nrx * out_stride + 64,), CANARY, dtype=torch.uint8, device="cuda")
        assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
        air.push(d_in.data_ptr() + pad * bsi, in_stride, c, d_out.data_ptr() + pad * bso, out_stride)
        keep.append((c, out_stride, d_in, d_out))
        at += c
    torch.cuda.synchronize()
    parts = []
    for c, out_stride, _, d_out in keep:
        o = d_out.cpu().numpy()
        assert (o[:pad * bso] == CANARY).all()
        rows = []
        for r in range(air.nrx):
            row = o[pad * bso + r * out_stride: pad * bso + (r + 1) * out_stride]
            assert (row[c * bso:] == CANARY).all(), f"receiver {r}: bytes stored past the call's {c} samples"
            rows.append(row[:c * bso])
        assert (o[pad * bso + air.nrx * out_stride:] == CANARY).all()
        parts.append(np.stack(rows))
    return np.concatenate(parts, axis=1)


def _cf32(row):
    return np.ascontiguousarray(row).view(np.float32).reshape(-1, 2).astype(np.float64)


def _check(out_fmt, row, y, b, tag):
    """the per-sample rule of contract 1 on one receiver's row; b: the bound, a scalar or one value per sample. Returns the largest
    error / bound (cf32) or the share of components inside a tie window (u8)."""
    b = np.asarray(b, dtype=np.float64)
    bb = b[:, None] if b.ndim else b
    if out_fmt == "cf32":
        e = np.abs(_cf32(row) - np.stack([y.real, y.imag], axis=-1))
        assert (e <= bb).all(), (tag, float(e.max()), float(np.max(b)))
        return float(np.max(e / np.maximum(bb, 1e-300)))
    got = row.reshape(-1, 2).astype(np.int64)
    q, v = airref.quantise_u8(y)
    d = np.abs(got - q)
    assert d.max(initial=0) <= 1, (tag, int(d.max()))
    window = airref.tie_window(v, b)
    assert not (d[~window] != 0).any(), (tag, int((d[~window] != 0).sum()))
    return float(window.mean())


# ---------------------------------------------------------------- 1. the model

CASES = [(Fs, i, o) for Fs in sh.FSS for i, o in sh.FORMATS]


@pytest.mark.parametrize("Fs,in_fmt,out_fmt", CASES, ids=[f"{Fs}-{i}-{o}" for Fs, i, o in CASES])
def test_air_matches_float64(built_lib, Fs, in_fmt, out_fmt):
    """three transmitters, four receivers (tests/airshapes.py), the starts 0, Fs - 5 and 2^31 + 3, without and with noise, in two calls:
    the second reads the first samples of every delay from the rings"""
    import pirip_amd
    x, paths = sh.inputs(Fs, in_fmt)
    xw = airref.widen(x, sh.FMT[in_fmt])
    air = pirip_amd.HipAir(Fs, paths, sh.NTX, sh.NRX, seed=sh.SEED, in_format=_fmt(in_fmt), out_format=_fmt(out_fmt))
    assert (air.ntx, air.nrx, air.max_delay, air.info.npaths) == (sh.NTX, sh.NRX, 4097, len(paths))
    assert (air.in_bytes_per_sample, air.out_bytes_per_sample) == (sh.BS[in_fmt], sh.BS[out_fmt])
    for k, n0 in enumerate(sh.starts(Fs)):
        clean = [airref.signal(xw, Fs, paths, r, n0) for r in range(sh.NRX)]
        for sigma in (None, sh.SIGMA):
            air.set_sigma(sigma)
            air.reset(n0)
            rows = _run(air, x, sh.CALLS, pad=k % 2)
            for r in range(sh.NRX):
                s = 0.0 if sigma is None else sigma[r]
                nz = airref.noise(sh.SEED, r, n0, sh.N, s)
                b = airref.bound(xw, paths, r, np.abs(nz)) if s else airref.bound(xw, paths, r)
                fig = _check(out_fmt, rows[r], clean[r] + nz, b, (Fs, in_fmt, out_fmt, n0, s, r))
                print(f"Fs {Fs} {in_fmt}->{out_fmt} n0 {n0} sigma {s} receiver {r}: "
                      + (f"largest error / bound {fig:.3f}" if out_fmt == "cf32" else f"share of components inside a tie window {fig:.2e}"))
                if not airref.paths_of(paths, r) and not s:                   # no path, no noise: all zeros / all bytes 128
                    assert (rows[r] == (0 if out_fmt == "cf32" else 128)).all()


def test_u8_identity_and_zero_history(built_lib):
    """u8 -> u8 through one path of gain 1 is the identity on all 256 byte values; before the start the input is zero -- byte 127.5, which
    the quantiser's tie sends to 128 --, not byte 128's value"""
    import pirip_amd
    b = np.arange(256)
    x = np.tile(np.stack([b, b[::-1]], axis=-1).astype(np.uint8), (9, 1))[None]          # 2304 samples: more than a tile
    air = pirip_amd.HipAir(240000, [(0, 0, 1.0, 0, 0), (1, 0, 1.0, 5, 0), (2, 0, 127.0, 3, 0)], 1, 3)
    rows = _run(air, x, [x.shape[1]]).reshape(3, -1, 2)
    assert np.array_equal(rows[0], x[0])
    assert np.array_equal(rows[1, 5:], x[0, :-5]) and (rows[1, :5] == 128).all()
    # gain 127 turns byte 128's 1 / 255 into half a level and more; a zero stays at 127.5 -> 128
    assert (rows[2, :3] == 128).all()
    assert np.array_equal(rows[2, 3:], airref.quantise_u8(airref.receive(airref.widen(x, airref.U8), 240000, [(0, 0, 127.0, 3, 0)], 0, 0))[0][3:])
    air.reset(77)                                                                         # and again after a reset: the ring is forgotten
    assert np.array_equal(_run(air, x, [100, x.shape[1] - 100], pad=1).reshape(3, -1, 2)[1], rows[1])


# ---------------------------------------------------------------- 2. cutting

@pytest.mark.parametrize("in_fmt,out_fmt", sh.FORMATS, ids=[f"{i}-{o}" for i, o in sh.FORMATS])
def test_any_cutting_equals_one_shot(built_lib, in_fmt, out_fmt):
    import pirip_amd
    Fs = 240000
    paths = sh.cut_paths(Fs)
    x, _ = sh.inputs(Fs, in_fmt, n=sh.CUT_N, ntx=2, seed=50)
    cuts = sh.CUTS + [sh.CUT_N - sum(sh.CUTS)]
    air = pirip_amd.HipAir(Fs, paths, 2, 2, sigma=[0.05, 0.08], seed=9, in_format=_fmt(in_fmt), out_format=_fmt(out_fmt))
    air.reset(sh.CUT_START)
    whole = _run(air, x, [sh.CUT_N])
    for pad in (0, 1):
        air.reset(sh.CUT_START)
        assert np.array_equal(_run(air, x, cuts, pad=pad), whole), pad
    air.reset(sh.CUT_START)
    assert np.array_equal(_run(air, x, [sh.CUT_N], pad=1), whole)
    air.reset(sh.CUT_START)
    assert np.array_equal(_run(air, x, cuts[::-1]), whole)                   # the long call first
    # and it is the model's (receiver 0 has three paths, two of them rotated)
    xw = airref.widen(x, sh.FMT[in_fmt])
    for r, s in enumerate((0.05, 0.08)):
        nz = airref.noise(9, r, sh.CUT_START, sh.CUT_N, s)
        _check(out_fmt, whole[r], airref.signal(xw, Fs, paths, r, sh.CUT_START) + nz, airref.bound(xw, paths, r, np.abs(nz)), (in_fmt, out_fmt, r))
    # without noise the start only counts modulo Fs
    air.set_sigma(None)
    air.reset(sh.CUT_START)
    quiet = _run(air, x, cuts)
    air.reset(sh.CUT_START + 3 * Fs)
    assert np.array_equal(_run(air, x, [sh.CUT_N]), quiet)
    air.reset(sh.CUT_START + 1)
    assert not np.array_equal(_run(air, x, [sh.CUT_N]), quiet)
    assert not np.array_equal(quiet, whole)


# ---------------------------------------------------------------- 3. noise

def test_noise_is_the_products_one_source(built_lib):
    """receivers with no path: the noise alone, the restatement's within its bound and HipTx.modulate's carrier-off rows bit for bit"""
    import torch
    import pirip_amd
    Fs, Rs, B, nsym, seed, sigma = 90000, 10000, 65, 300, 77, 0.6
    n = nsym * (Fs // Rs)
    x = np.zeros((1, n, 2), dtype=np.uint8)
    air = pirip_amd.HipAir(Fs, [], 1, B, sigma=sigma, seed=seed, out_format=pirip_amd.IN_CF32)
    rows = _run(air, x, [1000, n - 1000])
    for r in (0, 1, 63, 64):
        z = txref.noise_f64(seed, r, np.arange(n), sigma)
        got = _cf32(rows[r])
        err = np.maximum(np.abs(got[:, 0] - z.real), np.abs(got[:, 1] - z.imag))
        assert (err <= txref.NOISE_REL_BOUND * np.abs(z)).all(), (r, float(np.max(err / np.abs(z))))
    tx = pirip_amd.HipTx(pirip_amd.STANDIN_CODE, Fs, Rs, 2, nstreams=B, f1=10000, shift=10000)
    off = torch.full((B, nsym), txref.OFF, dtype=torch.uint8, device="cuda")
    out = torch.zeros((B, n * 8), dtype=torch.uint8, device="cuda")
    tx.modulate(off.data_ptr(), nsym, nsym, out.data_ptr(), n * 8, out_format=pirip_amd.IN_CF32, sigma=sigma, seed=seed)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), rows)
    # the u8 output of the same noise: the quantiser of the model's value
    air8 = pirip_amd.HipAir(Fs, [], 1, 2, sigma=[0.3, 0.0], seed=seed)
    r8 = _run(air8, x[:, :2100], [2100])
    z = txref.noise_f64(seed, 0, np.arange(2100), float(np.float32(0.3)))
    _check("u8", r8[0], z, airref.bound(airref.widen(x, airref.U8), [], 0, np.abs(z)), "u8 noise")
    assert (r8[1] == 128).all() and len(np.unique(r8[0])) > 100


def test_set_sigma_changes_the_calls_behind_it_only(built_lib):
    import pirip_amd
    Fs = 240000
    paths = sh.cut_paths(Fs)
    x, _ = sh.inputs(Fs, "u8", n=sh.CUT_N, ntx=2, seed=51)
    first, second = 1100, sh.CUT_N - 1100

    def run(s1, s2):
        import torch
        air = pirip_amd.HipAir(Fs, paths, 2, 2, sigma=s1, seed=4)
        ntx, n = 2, sh.CUT_N
        d_in = torch.from_numpy(np.ascontiguousarray(x).reshape(ntx, n * 2)).cuda()
        d_out = torch.zeros((2, n * 2), dtype=torch.uint8, device="cuda")
        air.push(d_in.data_ptr(), n * 2, first, d_out.data_ptr(), n * 2)
        air.set_sigma(s2)                                                        # enqueued: no synchronisation in between
        air.push(d_in.data_ptr() + first * 2, n * 2, second, d_out.data_ptr() + first * 2, n * 2)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()

    a, b, swept = run([0.02, 0.0], [0.02, 0.0]), run([0.2, 0.1], [0.2, 0.1]), run([0.02, 0.0], [0.2, 0.1])
    assert np.array_equal(swept[:, :first * 2], a[:, :first * 2]) and np.array_equal(swept[:, first * 2:], b[:, first * 2:])
    assert not np.array_equal(a, b)


# ---------------------------------------------------------------- 4. clipping

def test_clipping_is_the_adcs(built_lib):
    import pirip_amd
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, (2, sh.CLIP_N, 2)).astype(np.uint8)
    xw = airref.widen(x, airref.U8)
    y = airref.signal(xw, 240000, sh.CLIP_PATHS, 0, 0)
    b = airref.bound(xw, sh.CLIP_PATHS, 0)
    u8 = _run(pirip_amd.HipAir(240000, sh.CLIP_PATHS, 2, 1), x, [sh.CLIP_N])[0]
    _check("u8", u8, y, b, "overdriven u8")
    got = u8.reshape(-1, 2)
    _, v = airref.quantise_u8(y)
    assert (v < -10).any() and (v > 265).any() and (got[v < -1] == 0).all() and (got[v > 256] == 255).all() and (got == 0).any() and (got == 255).any()
    cf = _run(pirip_amd.HipAir(240000, sh.CLIP_PATHS, 2, 1, out_format=pirip_amd.IN_CF32), x, [sh.CLIP_N])[0]
    _check("cf32", cf, y, b, "overdriven cf32")
    assert _cf32(cf).max() > 2 and _cf32(cf).min() < -2                         # unclamped


# ---------------------------------------------------------------- 5. independence

@pytest.mark.parametrize("in_fmt,out_fmt", [("u8", "u8"), ("cf32", "cf32")])
def test_receiver_does_not_depend_on_the_others(built_lib, in_fmt, out_fmt):
    import pirip_amd
    Fs = 240000
    x, paths = sh.inputs(Fs, in_fmt)
    kw = dict(in_format=_fmt(in_fmt), out_format=_fmt(out_fmt), seed=sh.SEED)
    n0 = Fs - 5
    full = pirip_amd.HipAir(Fs, paths, sh.NTX, sh.NRX, sigma=sh.SIGMA, **kw)
    full.reset(n0)
    noisy = _run(full, x, sh.CALLS)
    full.set_sigma(None)
    full.reset(n0)
    quiet = _run(full, x, sh.CALLS)
    for r in range(sh.NRX):
        mine = airref.paths_of(paths, r)
        # beside receivers that hear nothing, at the same index: the noise is keyed by it
        alone = pirip_amd.HipAir(Fs, mine, sh.NTX, sh.NRX, sigma=sh.SIGMA, **kw)
        alone.reset(n0)
        assert np.array_equal(_run(alone, x, [sh.N], pad=1)[r], noisy[r]), r
        # as the only receiver, and in other company at another index, without noise
        single = pirip_amd.HipAir(Fs, [(0,) + p[1:] for p in mine], sh.NTX, 1, **kw)
        single.reset(n0)
        assert np.array_equal(_run(single, x, [sh.N])[0], quiet[r]), r
        other = pirip_amd.HipAir(Fs, [(0, 2, 1.0, 9, 77)] + [(2,) + p[1:] for p in mine] + [(1, 0, -1.0, 0, 0)], sh.NTX, 3, **kw)
        other.reset(n0)
        assert np.array_equal(_run(other, x, sh.CALLS[::-1])[2], quiet[r]), r


# ---------------------------------------------------------------- 6. limits

def test_limits_and_bad_arguments(built_lib):
    """every PIRIP_ERR_BAD_ARG / PIRIP_ERR_UNSUPPORTED line of the header, both sides of each"""
    import torch
    import pirip_amd
    A = pirip_amd.HipAir
    L = built_lib
    Fs = 240000
    one = [(0, 0, 1.0, 0, 0)]

    def fails(code, fn, *a, **kw):
        with pytest.raises(pirip_amd.PiripError, match=rf"\({code}\)"):
            fn(*a, **kw)

    def ok(*a, **kw):
        A(*a, **kw).close()

    fails(BAD_ARG, A, Fs, [], 0, 1); fails(BAD_ARG, A, Fs, [], 1, 0); ok(Fs, [], 1, 1)                          # ntx, nrx < 1; no path at all is fine
    h = C.c_void_p()
    p = pirip_amd.AirPath(0, 0, 0, 0, 1.0)
    assert L.pirip_hip_air_create(Fs, 1, 1, 1, 1, -1, C.addressof(p), None, 1, -1, C.byref(h)) == BAD_ARG        # npaths < 0
    assert L.pirip_hip_air_create(Fs, 1, 1, 1, 1, 1, None, None, 1, -1, C.byref(h)) == BAD_ARG                   # paths NULL
    assert L.pirip_hip_air_create(Fs, 1, 1, 1, 1, 1, C.addressof(p), None, 1, -1, None) == BAD_ARG               # out NULL
    fails(BAD_ARG, A, Fs, [(2, 0, 1.0, 0, 0)], 2, 2); fails(BAD_ARG, A, Fs, [(-1, 0, 1.0, 0, 0)], 2, 2); ok(Fs, [(1, 0, 1.0, 0, 0)], 2, 2)
    fails(BAD_ARG, A, Fs, [(0, 2, 1.0, 0, 0)], 2, 2); fails(BAD_ARG, A, Fs, [(0, -1, 1.0, 0, 0)], 2, 2); ok(Fs, [(0, 1, 1.0, 0, 0)], 2, 2)
    fails(BAD_ARG, A, Fs, [(0, 0, 1.0, -1, 0)], 1, 1); ok(Fs, one, 1, 1)                                         # delay < 0
    fails(BAD_ARG, A, Fs, [(0, 0, 1.0, 0, Fs // 2)], 1, 1); fails(BAD_ARG, A, Fs, [(0, 0, 1.0, 0, -Fs // 2)], 1, 1)
    ok(Fs, [(0, 0, 1.0, 0, Fs // 2 - 1), (0, 0, 1.0, 0, -(Fs // 2 - 1))], 1, 1)
    fails(BAD_ARG, A, Fs + 1, [(0, 0, 1.0, 0, Fs // 2 + 1)], 1, 1); ok(Fs + 1, [(0, 0, 1.0, 0, Fs // 2), (0, 0, 1.0, 0, -(Fs // 2))], 1, 1)   # an odd rate
    for bad in (float("nan"), float("inf"), -float("inf")):
        fails(BAD_ARG, A, Fs, [(0, 0, bad, 0, 0)], 1, 1)
        fails(BAD_ARG, A, Fs, one, 1, 1, sigma=bad)
    fails(BAD_ARG, A, Fs, one, 1, 1, sigma=-1e-6); ok(Fs, one, 1, 1, sigma=0.0); ok(Fs, [(0, 0, -3e38, 0, 0)], 1, 1, sigma=3e38)
    fails(BAD_ARG, A, 1, one, 1, 1); ok(2, one, 1, 1)                                                            # Fs < 2
    for fmt in (pirip_amd.IN_CU8_FSKDEMOD, pirip_amd.IN_CS16, 4, -1):
        fails(BAD_ARG, A, Fs, one, 1, 1, in_format=fmt)
        fails(BAD_ARG, A, Fs, one, 1, 1, out_format=fmt)
    fails(UNSUPPORTED, A, (1 << 24) + 1, one, 1, 1); ok(1 << 24, one, 1, 1)
    fails(UNSUPPORTED, A, Fs, [(0, 0, 1.0, (1 << 20) + 1, 0)], 1, 1)
    fails(UNSUPPORTED, A, Fs, one, 1, 65536); ok(Fs, one, 1, 65535)
    fails(UNSUPPORTED, A, Fs, one, 65536, 1); ok(Fs, one, 65535, 1)
    with pytest.raises(ValueError):
        A(Fs, one, 1, 2, sigma=[0.1, 0.2, 0.3])

    # the longest delay allowed, in use: the second call reads 2^20 samples back
    far = A(Fs, [(0, 0, 1.0, 1 << 20, 0)], 1, 1)
    assert far.max_delay == 1 << 20
    n = (1 << 20) + 300
    rng = np.random.default_rng(12)
    x = rng.integers(0, 256, (1, n, 2)).astype(np.uint8)
    got = _run(far, x, [1 << 20, 300]).reshape(-1, 2)
    assert (got[:1 << 20] == 128).all() and np.array_equal(got[1 << 20:], x[0, :300])

    # push
    air = A(Fs, [(0, 0, 1.0, 3, 0), (1, 1, 1.0, 0, 0)], 2, 2)
    cf = A(Fs, [(0, 0, 1.0, 3, 0), (1, 1, 1.0, 0, 0)], 2, 2, in_format=pirip_amd.IN_CF32, out_format=pirip_amd.IN_CF32)
    d_in = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    i, o = d_in.data_ptr(), d_out.data_ptr()
    fails(BAD_ARG, air.push, i, 1024, 0, o, 1024); fails(BAD_ARG, air.push, i, 1024, -1, o, 1024)                # n < 1
    fails(BAD_ARG, air.push, 0, 1024, 10, o, 1024); fails(BAD_ARG, air.push, i, 1024, 10, 0, 1024)               # NULL
    fails(BAD_ARG, air.push, i + 1, 1024, 10, o, 1024); fails(BAD_ARG, air.push, i, 1023, 10, o, 1024)           # rows off the sample
    fails(BAD_ARG, air.push, i, 1024, 10, o + 1, 1024); fails(BAD_ARG, air.push, i, 1024, 10, o, 1023)
    fails(BAD_ARG, cf.push, i + 4, 1024, 10, o, 1024); fails(BAD_ARG, cf.push, i, 1028, 10, o, 1024)
    fails(BAD_ARG, cf.push, i, 1024, 10, o + 4, 1024); fails(BAD_ARG, cf.push, i, 1024, 10, o, 1028)
    fails(BAD_ARG, air.push, i, 18, 10, o, 1024); fails(BAD_ARG, air.push, i, 1024, 10, o, 18)                   # rows of one side overlap
    air.push(i, 20, 10, o, 20)                                                                                   # ... and just do not
    fails(BAD_ARG, air.push, i, 1024, 10, i, 1024); fails(BAD_ARG, air.push, i, 1024, 10, i + 1024 + 18, 1024)   # d_out overlaps d_in
    fails(BAD_ARG, air.push, i + 1044 - 2, 1024, 10, i, 1024)
    air.push(i, 1024, 10, i + 1024 + 20, 1024); air.push(i + 1044, 1024, 10, i, 1024)                            # ... and lies just beside it
    air.push(i, 1024, 1, o, 1024); cf.push(i, 1024, 1, o, 1024)                                                  # n = 1
    air.push(i + 2, 1026, 10, o + 6, 1022); cf.push(i + 8, 1032, 10, o + 24, 1016)                               # aligned to the sample only
    # the absolute index stays below 2^53
    fails(BAD_ARG, air.reset, -1); fails(UNSUPPORTED, air.reset, 1 << 53); air.reset((1 << 53) - 1)
    fails(UNSUPPORTED, air.push, i, 1024, 1, o, 1024)
    air.reset((1 << 53) - 11)
    fails(UNSUPPORTED, air.push, i, 1024, 11, o, 1024)
    air.push(i, 1024, 10, o, 1024)
    fails(UNSUPPORTED, air.push, i, 1024, 1, o, 1024)
    # set_sigma
    assert L.pirip_hip_air_set_sigma(air.h, None, None) == BAD_ARG
    for bad in (float("nan"), float("inf"), -0.5):
        fails(BAD_ARG, air.set_sigma, [0.0, bad])
    air.set_sigma([0.0, 0.5])
    with pytest.raises(ValueError):
        air.set_sigma([0.1, 0.2, 0.3])
    info = pirip_amd.AirInfo()
    assert L.pirip_hip_air_get_info(air.h, None) == BAD_ARG and L.pirip_hip_air_get_info(None, C.byref(info)) == BAD_ARG
    assert L.pirip_hip_air_destroy(None) == BAD_ARG
    torch.cuda.synchronize()


def test_the_last_samples_below_two_to_the_53(built_lib):
    """the model at the largest start there is"""
    import pirip_amd
    Fs, n = 240000, 2100
    n0 = (1 << 53) - 1 - n
    paths = [(0, 0, 0.4, 70, 12345), (0, 0, -0.3, 0, -1)]
    rng = np.random.default_rng(13)
    x = rng.integers(0, 256, (1, n, 2)).astype(np.uint8)
    xw = airref.widen(x, airref.U8)
    air = pirip_amd.HipAir(Fs, paths, 1, 1, sigma=0.05, seed=3, out_format=pirip_amd.IN_CF32)
    air.reset(n0)
    row = _run(air, x, [1000, n - 1000])[0]
    nz = airref.noise(3, 0, n0, n, 0.05)
    _check("cf32", row, airref.signal(xw, Fs, paths, 0, n0) + nz, airref.bound(xw, paths, 0, np.abs(nz)), "2^53")


# ---------------------------------------------------------------- 7. the shared-medium loop

@pytest.fixture(scope="module")
def medium(built_lib):
    """tests/test_ping.py's terminal and repeater, joined by one channel instead of a wire: per call the channel takes what both ends
    sent in the call before (silence at first) and gives each end what it hears -- the other end through the far path, itself through
    the leak, and its own noise."""
    import torch
    import pirip_amd
    from test_ping import LOOP_CALLS, _Repeater, _Terminal
    term, rep = _Terminal(), _Repeater()
    block, blk, K = term.block, term.block * 2, LOOP_CALLS
    assert rep.block == block and sh.FAR["delay"] < block
    air = pirip_amd.HipAir(ms.LOOP["Fs"], sh.LOOP_PATHS, 2, 2, sigma=sh.LOOP_SIGMA, seed=sh.LOOP_SEED)
    sent = torch.full((K + 1, 2, blk), 128, dtype=torch.uint8, device="cuda")           # [k + 1]: what terminal and repeater sent in call k
    heard = torch.zeros((K, 2, blk), dtype=torch.uint8, device="cuda")
    for k in range(K):
        air.push(sent[k], blk, block, heard[k], blk)
        term.ping.push(heard[k, 0], blk, sent[k + 1, 0], blk)
        rep.rpt.push(heard[k, 1], blk, sent[k + 1, 1], blk)
    torch.cuda.synchronize()
    return dict(term=term, rep=rep, air=air, sent=sent, heard=heard, logs=[term.ping.log(c) for c in range(4)], ping=term.ping.counters(),
                rpt=rep.rpt.counters())


def test_shared_medium_loop(medium):
    """Far paths of gain 1, 1234 samples late and 137 Hz up, leaks of gain 0.5, sigma 0.1 at both receivers: about 25 dB Eb/N0 on the far
    path and 19 dB on the leak for the weakest channel, far above the code's threshold (tests/test_air_cpu.py decodes both legs on the
    reference chain). The terminal logs the repeater's three frames per channel and filters its own three; the repeater repeats one burst
    per channel and filters its own reply."""
    nfr = ms.LOOP["nframes"]
    c, rc = medium["ping"], medium["rpt"]
    for ch in range(4):
        log = medium["logs"][ch]
        assert len(log) == nfr, (ch, log)
        assert log["source"].tolist() == [2] * nfr and log["seq"].tolist() == [1, 2, 3] and not log["ecdd"].any(), (ch, log)
    assert c["frames"].tolist() == [nfr] * 4 and c["filtered"].tolist() == [nfr] * 4
    assert c["bursts_sent"].tolist() == [1] * 4 and c["frames_sent"].tolist() == [nfr] * 4
    assert not c["lost"].any() and not c["skipped"].any() and not c["bit_errors"].any()
    assert rc["bursts_in"].tolist() == [1] * 4 and rc["bursts_out"].tolist() == [1] * 4 and rc["filtered"].tolist() == [nfr] * 4
    # the medium did something: both ends heard noise on every sample's neighbourhood, and nothing of it was a wire
    heard, sent = medium["heard"].cpu().numpy(), medium["sent"].cpu().numpy()
    assert len(np.unique(heard[0])) > 50 and not np.array_equal(heard[5, 0], sent[5, 1])


def test_what_each_end_heard_is_the_models(medium):
    """one block in the middle of the repeater's reply, both receivers: the channel's bytes are the float64 statement's on what was sent"""
    sent, heard = medium["sent"].cpu().numpy(), medium["heard"].cpu().numpy()
    block = medium["term"].block
    busy = [k for k in range(1, heard.shape[0]) if (sent[k - 1:k + 1, 1] != 128).any() and (sent[k - 1:k + 1, 0] != 128).any()]
    k = busy[len(busy) // 2] if busy else next(k for k in range(1, heard.shape[0]) if (sent[k] != 128).any())
    # the block before supplies the delayed samples
    x = np.concatenate([sent[k - 1], sent[k]], axis=1).reshape(2, 2 * block, 2)
    xw = airref.widen(x, airref.U8)
    for r in range(2):
        n0 = (k - 1) * block
        nz = airref.noise(sh.LOOP_SEED, r, n0, 2 * block, sh.LOOP_SIGMA)
        y = airref.signal(xw, ms.LOOP["Fs"], sh.LOOP_PATHS, r, n0) + nz
        b = airref.bound(xw, sh.LOOP_PATHS, r, np.abs(nz))
        _check("u8", heard[k, r], y[block:], b[block:], ("loop", k, r))


# ---------------------------------------------------------------- 8. the command-line tool

@pytest.mark.parametrize("in_fmt,out_fmt", [("u8", "cf32"), ("cf32", "u8")])
def test_cli_equals_the_binding(built_lib, tmp_path, in_fmt, out_fmt):
    import pirip_amd
    Fs, start = 240000, 2 ** 31 + 3
    paths = sh.cut_paths(Fs)
    x, _ = sh.inputs(Fs, in_fmt, n=sh.CUT_N, ntx=2, seed=52)
    names = [str(tmp_path / f"{d}{i}") for d in ("in", "out") for i in range(2)]
    x[0].tofile(names[0])
    x[1, :sh.CUT_N - 7].tofile(names[1])                                       # the shortest input decides
    n = sh.CUT_N - 7
    cmd = [os.path.join(ms.BIN, "air_channels"), "--fs", str(Fs), "--in-format", in_fmt, "--out-format", out_fmt, "--sigma", "0.05,0.08", "--seed", "9",
           "--block", "1000", "--start", str(start), "-q"]
    for rx, tx, g, d, f in paths:
        cmd += ["--path", f"{rx},{tx},{g:.9g},{d},{f}"]
    p = subprocess.run(cmd + names[:2] + ["--"] + names[2:], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    air = pirip_amd.HipAir(Fs, paths, 2, 2, sigma=[0.05, 0.08], seed=9, in_format=_fmt(in_fmt), out_format=_fmt(out_fmt))
    air.reset(start)
    want = _run(air, x[:, :n], [n])
    for r in range(2):
        got = np.fromfile(names[2 + r], dtype=np.uint8)
        assert got.size == n * sh.BS[out_fmt] and np.array_equal(got, want[r]), r
    assert (want[0] != want[1]).any()
    # what the tool refuses
    bad = subprocess.run(cmd[:3] + ["--path", "0,0,1.0,0"] + names[:1] + ["--"] + names[2:3], capture_output=True, timeout=60)
    assert bad.returncode == 1
    bad = subprocess.run(cmd[:3] + ["--path", "0,5,1.0,0,0"] + names[:1] + ["--"] + names[2:3], capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"channel" in bad.stderr
