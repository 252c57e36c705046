"""include/pirip_hip.h section O, fading: paths whose gain moves, Rayleigh or Rician with a Doppler spread (pirip_hip_air_create_fade,
pirip_amd.HipAir(fades=...)), on the device.

Contract 1: every complex-float component within faderef.bound -- driftref.bound with Gamma L max |x| for a fading path's |x| and the
fade's own terms, derived in DESIGN.md 4.15b -- of the float64 statement (tests/faderef.py) on the library's own tables; u8 bytes within
one level of the quantised model and different from it only inside airref.tie_window of that bound. Contract 2, bit for bit: any cutting
into calls equals one shot, n0 equals n0 + 2^32 without noise, drift and carrier offsets, a handle of pirip_hip_air_create_fade without a
fade equals pirip_hip_air_create_ex's and pirip_hip_air_create's, a receiver does not depend on another receiver's fades. Contract 3: the
demodulator holds the test bits through a Rayleigh and a Rician path wherever the oracle does on the model, and terminal and repeater find
each other over a medium whose far paths fade. tests/test_air_fade_cpu.py shows on the model alone that the inputs used here reach what
they claim."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import airref
import airshapes as sh
import faderef
import fadeshapes as fs
import muxshapes as ms
import sigutil
from test_air import _cf32, _check, _fmt, _run

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. the model

CASES = [(Fs, i, o) for Fs in fs.FSS for i, o in fs.FORMATS]


@pytest.mark.parametrize("Fs,in_fmt,out_fmt", CASES, ids=[f"{Fs}-{i}-{o}" for Fs, i, o in CASES])
def test_fade_matches_float64(built_lib, Fs, in_fmt, out_fmt):
    """fadeshapes.layout -- static, fading static, fading rotated at +-(Fs/2 - 1), fading drifting at +-300000 ppb, two fading paths of one
    transmitter at delays 1 and 65, Doppler 0 and the Doppler limit, K 0, 1 and 10^6 -- in two calls, without and with noise, from every
    start of fadeshapes.STARTS. The K = 10^6 receiver's complex-float output is also held to the same path without a fade, within the
    bound and |a| max |x| (1 - los + 16 s)."""
    import pirip_amd
    x, paths, fades = fs.inputs(Fs, in_fmt)
    xw = airref.widen(x, fs.FMT[in_fmt])
    air = pirip_amd.HipAir(Fs, paths, fs.NTX, fs.NRX, seed=fs.SEED, in_format=_fmt(in_fmt), out_format=_fmt(out_fmt), max_slip=fs.MAX_SLIP, fades=fades)
    assert air.info.npaths == len(paths) and air.drift()[0] == fs.MAX_SLIP and len(air.fades) == len(fades)
    los_path = next(i for i, p in enumerate(paths) if p[0] == 2)
    tab = faderef.table(Fs, fs.SEED, faderef.fade_on(fades, los_path))
    los_slack = abs(paths[los_path][2]) * float(np.abs(xw[paths[los_path][1]]).max()) * (1.0 - tab[3] + 16 * tab[2])
    worst = 0.0
    for k, n0 in enumerate(fs.STARTS):
        clean = [faderef.signal(xw, Fs, paths, fades, fs.SEED, r, n0) for r in range(fs.NRX)]
        for sigma in (None, fs.SIGMA):
            air.set_sigma(sigma)
            air.reset(n0)
            rows = _run(air, x, fs.CALLS, pad=k % 2)
            for r in range(fs.NRX):
                s = 0.0 if sigma is None else sigma[r]
                nz = airref.noise(fs.SEED, r, n0, fs.N, s)
                b = faderef.bound(xw, Fs, paths, fades, fs.SEED, r, np.abs(nz)) if s else faderef.bound(xw, Fs, paths, fades, fs.SEED, r)
                fig = _check(out_fmt, rows[r], clean[r] + nz, b, (Fs, in_fmt, out_fmt, n0, s, r))
                print(f"Fs {Fs} {in_fmt}->{out_fmt} n0 {n0} sigma {s} receiver {r}: "
                      + (f"largest error / bound {fig:.3f}" if out_fmt == "cf32" else f"share of components inside a tie window {fig:.2e}"))
                if out_fmt == "cf32":
                    worst = max(worst, fig)
            if out_fmt == "cf32":                                      # receiver 2 (sigma 0 in both runs) against its path without a fade
                plain = airref.signal(xw, Fs, [paths[los_path][:5]], 2, n0)
                e = np.abs(_cf32(rows[2]) - np.stack([plain.real, plain.imag], axis=-1))
                assert (e <= faderef.bound(xw, Fs, paths, fades, fs.SEED, 2) + los_slack).all(), (n0, float(e.max()), los_slack)
    air.close()
    if out_fmt == "cf32":
        print(f"Fs {Fs} {in_fmt}->{out_fmt}: largest error / bound of the case {worst:.3f}")


# ---------------------------------------------------------------- 2. a period of 2^32 samples

def test_start_counts_modulo_two_to_the_32(built_lib):
    """sigma 0, no drifting path, every carrier offset 0: the starts 5 and 2^32 + 5 give the same bytes (the phases take the index modulo
    2^32), a start half a period on does not"""
    import pirip_amd
    Fs = 240000
    x, _ = sh.inputs(Fs, "u8", n=fs.N, ntx=2, seed=70)
    for out_fmt in ("u8", "cf32"):
        air = pirip_amd.HipAir(Fs, fs.WRAP_PATHS, 2, 2, seed=3, out_format=_fmt(out_fmt), fades=fs.WRAP_FADES)
        got = []
        for n0 in (5, 2 ** 32 + 5, 2 ** 31 + 5):
            air.reset(n0)
            got.append(_run(air, x, fs.CALLS))
        assert np.array_equal(got[0], got[1]) and not np.array_equal(got[0][0], got[2][0])
        assert np.array_equal(got[0][1], got[2][1])                     # receiver 1's one path has no fade: the start does not count at all


# ---------------------------------------------------------------- 3. cutting

@pytest.mark.parametrize("in_fmt,out_fmt", fs.FORMATS, ids=[f"{i}-{o}" for i, o in fs.FORMATS])
def test_any_cutting_equals_one_shot_under_fading(built_lib, in_fmt, out_fmt):
    import pirip_amd
    Fs = 240000
    paths, fades = fs.cut_paths(Fs)
    x, _ = sh.inputs(Fs, in_fmt, n=fs.CUT_N, ntx=2, seed=60)
    cuts = fs.CUTS + [fs.CUT_N - sum(fs.CUTS)]
    air = pirip_amd.HipAir(Fs, paths, 2, 2, sigma=fs.CUT_SIGMA, seed=fs.CUT_SEED, in_format=_fmt(in_fmt), out_format=_fmt(out_fmt), max_slip=fs.CUT_SLIP,
                           fades=fades)
    air.reset(fs.CUT_START, age=fs.CUT_AGE)
    whole = _run(air, x, [fs.CUT_N])
    for pad in (0, 1):
        air.reset(fs.CUT_START, age=fs.CUT_AGE)
        assert np.array_equal(_run(air, x, cuts, pad=pad), whole), pad
    air.reset(fs.CUT_START, age=fs.CUT_AGE)
    assert np.array_equal(_run(air, x, [fs.CUT_N], pad=1), whole)
    air.reset(fs.CUT_START, age=fs.CUT_AGE)
    assert np.array_equal(_run(air, x, cuts[::-1]), whole)                   # the long call first
    # and it is the model's
    xw = airref.widen(x, fs.FMT[in_fmt])
    for r, s in enumerate(fs.CUT_SIGMA):
        nz = airref.noise(fs.CUT_SEED, r, fs.CUT_START, fs.CUT_N, s)
        _check(out_fmt, whole[r], faderef.signal(xw, Fs, paths, fades, fs.CUT_SEED, r, fs.CUT_START, age0=fs.CUT_AGE) + nz,
               faderef.bound(xw, Fs, paths, fades, fs.CUT_SEED, r, np.abs(nz)), (in_fmt, out_fmt, r))
    # the gain is the receiver's index's: one sample on, other bytes
    air.reset(fs.CUT_START + 1, age=fs.CUT_AGE)
    assert not np.array_equal(_run(air, x, [fs.CUT_N]), whole)


# ---------------------------------------------------------------- 4. no change

def _create_fade_without_fades(Fs, paths, ntx, nrx, max_slip=0, **kw):
    """a HipAir whose handle pirip_hip_air_create_fade made with nfades = 0 (the binding never calls it without a fade)"""
    import pirip_amd
    air = pirip_amd.HipAir(Fs, paths, ntx, nrx, max_slip=max_slip, **kw)
    air.close()
    arr = (pirip_amd.AirPathEx * len(paths))()
    for i, p in enumerate(paths):
        arr[i] = pirip_amd.AirPathEx(int(p[0]), int(p[1]), int(p[3]), int(p[4]), float(p[2]), int(p[5]) if len(p) > 5 else 0)
    sg = pirip_amd.HipAir._sigma(kw.get("sigma"), nrx)
    h = C.c_void_p()
    rc = air.L.pirip_hip_air_create_fade(Fs, kw.get("in_format", pirip_amd.IN_CU8_CSDR), kw.get("out_format", pirip_amd.IN_CU8_CSDR), ntx, nrx, len(paths),
                                         C.addressof(arr), 0, None, None if sg is None else sg.ctypes.data, int(kw.get("seed", 1)), max_slip, -1,
                                         C.byref(h))
    assert rc == 0, rc
    air.h = h
    return air


@pytest.mark.parametrize("in_fmt,out_fmt", fs.FORMATS, ids=[f"{i}-{o}" for i, o in fs.FORMATS])
def test_without_a_fade_nothing_changes(built_lib, in_fmt, out_fmt):
    """pirip_hip_air_create_fade with nfades = 0 gives pirip_hip_air_create_ex's bytes with drifting paths and pirip_hip_air_create's without;
    and a receiver without a fade does not depend on another receiver's fades, which put the whole handle on the other kernel (canaries round
    every row)"""
    import pirip_amd
    Fs, n0 = 240000, 240000 - 5
    kw = dict(sigma=sh.SIGMA, seed=sh.SEED, in_format=_fmt(in_fmt), out_format=_fmt(out_fmt))
    x, paths = sh.inputs(Fs, in_fmt)
    plain = pirip_amd.HipAir(Fs, paths, sh.NTX, sh.NRX, **kw)
    plain.reset(n0)
    want = _run(plain, x, sh.CALLS)
    none = _create_fade_without_fades(Fs, paths, sh.NTX, sh.NRX, **kw)
    none.reset(n0)
    assert np.array_equal(_run(none, x, sh.CALLS, pad=1), want)
    # with clock offsets: pirip_hip_air_create_ex
    drifting = [p + (0,) for p in paths] + [(0, 0, 0.1, 40, 77, 300000), (0, 1, -0.1, 9, 0, -1000000)]
    ex = pirip_amd.HipAir(Fs, drifting, sh.NTX, sh.NRX, max_slip=20, **kw)
    ex.reset(n0, age=2000)
    budget = ex.drift()
    want_ex = _run(ex, x, sh.CALLS)
    none = _create_fade_without_fades(Fs, drifting, sh.NTX, sh.NRX, max_slip=20, **kw)
    none.reset(n0, age=2000)
    assert none.drift() == budget
    assert np.array_equal(_run(none, x, sh.CALLS), want_ex)
    # receiver 0 of airshapes' layout has no path: give it fading ones, a drifting one among them; and fade one path of receiver 2
    extra = [(0, 0, 0.02, 40, 77, 300000), (0, 1, -0.02, 9, 0, 0)]
    for lay, base, slip, age in ((paths, want, 0, 0), (drifting, want_ex, 20, 2000)):
        m = len(lay)
        mixed = pirip_amd.HipAir(Fs, [p[:5] + (p[5] if len(p) > 5 else 0,) for p in lay] + extra, sh.NTX, sh.NRX, max_slip=max(slip, 20),
                                 fades=[(m, 20.0, 0.0, 1), (m + 1, 7.0, 4.0, 2), (1, 20.0, 1.0, 3)], **kw)
        mixed.reset(n0, age=age)
        got = _run(mixed, x, sh.CALLS)
        assert paths[1][0] == 2
        assert np.array_equal(got[1], base[1]) and np.array_equal(got[3], base[3])
        assert not np.array_equal(got[0], base[0]) and not np.array_equal(got[2], base[2])


# ---------------------------------------------------------------- 5. a level sweep

def test_set_sigma_between_two_calls_on_a_fading_handle(built_lib):
    import pirip_amd
    Fs = 240000
    paths, fades = fs.cut_paths(Fs)
    x, _ = sh.inputs(Fs, "u8", n=fs.CUT_N, ntx=2, seed=51)
    first, second = 1100, fs.CUT_N - 1100

    def run(s1, s2):
        import torch
        air = pirip_amd.HipAir(Fs, paths, 2, 2, sigma=s1, seed=4, max_slip=fs.CUT_SLIP, fades=fades)
        ntx, n = 2, fs.CUT_N
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


# ---------------------------------------------------------------- 6. demodulation on the device

def test_demodulator_holds_the_test_bits_through_fading_paths(built_lib, oracle):
    """tests/test_air_fade_cpu.py's signal through HipAir (u8 -> u8, receiver 0 over a Rayleigh path of 20 Hz, receiver 1 over a Rician
    one) into HipDemod: the same frames count, and every one of them after the first is a stretch of the test bits without an error"""
    import pirip_amd
    c = sigutil.CFG1
    u8, bits = fs.demod_input(oracle)
    air = pirip_amd.HipAir(c["Fs"], fs.DEMOD_PATHS, 1, 2, seed=fs.DEMOD_SEED, fades=fs.DEMOD_FADES)
    n = u8.shape[0]
    rows = _run(air, u8[None], [n // 2 + 11, n - n // 2 - 11]).reshape(2, n, 2)
    idx = np.arange(n, dtype=np.int64)
    for r, name in enumerate(("rayleigh", "rician")):
        gmag = np.abs(faderef.gain(faderef.table(c["Fs"], fs.DEMOD_SEED, fs.DEMOD_FADES[r]), idx))
        h = pirip_amd.HipDemod(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=c["est_min"], est_max=c["est_max"], nstreams=1)
        rh = h.demod_host(np.ascontiguousarray(rows[r]))
        frames, out, bad = fs.demod_check(rh, h.N + 2 * (c["Fs"] // c["Rs"]), bits, gmag)
        print(f"{name}: {frames} frames, {out} left out, frames with errors {bad}")
        assert frames >= 35 and out <= (frames - 1) / 5 and not bad


# ---------------------------------------------------------------- 7. the shared-medium loop over fading far paths

@pytest.fixture(scope="module")
def medium(built_lib):
    """tests/test_air.py's medium with Rician far paths (K = 4, 5 Hz); the leaks stay as they are"""
    import torch
    import pirip_amd
    from test_ping import LOOP_CALLS, _Repeater, _Terminal
    term, rep = _Terminal(), _Repeater()
    block, blk, K = term.block, term.block * 2, LOOP_CALLS
    assert rep.block == block and sh.FAR["delay"] < block
    air = pirip_amd.HipAir(ms.LOOP["Fs"], fs.LOOP_PATHS, 2, 2, sigma=sh.LOOP_SIGMA, seed=sh.LOOP_SEED, fades=fs.LOOP_FADES)
    sent = torch.full((K + 1, 2, blk), 128, dtype=torch.uint8, device="cuda")
    heard = torch.zeros((K, 2, blk), dtype=torch.uint8, device="cuda")
    for k in range(K):
        air.push(sent[k], blk, block, heard[k], blk)
        term.ping.push(heard[k, 0], blk, sent[k + 1, 0], blk)
        rep.rpt.push(heard[k, 1], blk, sent[k + 1, 1], blk)
    torch.cuda.synchronize()
    return dict(term=term, rep=rep, air=air, sent=sent, heard=heard, logs=[term.ping.log(c) for c in range(4)], ping=term.ping.counters(),
                rpt=rep.rpt.counters())


def test_shared_medium_loop_over_fading_paths(medium):
    """tests/test_air.py's test_shared_medium_loop, same expectations: three frames logged per channel, numbered 1, 2, 3 with ecdd 0; own
    frames filtered; one repeated burst per channel"""
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


def test_what_each_end_heard_over_fading_paths_is_the_models(medium):
    """one busy block, both receivers: the channel's bytes are the float64 statement's at that block's absolute index"""
    sent, heard = medium["sent"].cpu().numpy(), medium["heard"].cpu().numpy()
    block = medium["term"].block
    busy = [k for k in range(1, heard.shape[0]) if (sent[k - 1:k + 1, 1] != 128).any() and (sent[k - 1:k + 1, 0] != 128).any()]
    k = busy[len(busy) // 2] if busy else next(k for k in range(1, heard.shape[0]) if (sent[k] != 128).any())
    x = np.concatenate([sent[k - 1], sent[k]], axis=1).reshape(2, 2 * block, 2)
    xw = airref.widen(x, airref.U8)
    n0 = (k - 1) * block
    Fs = ms.LOOP["Fs"]
    for r in range(2):
        nz = airref.noise(sh.LOOP_SEED, r, n0, 2 * block, sh.LOOP_SIGMA)
        y = faderef.signal(xw, Fs, fs.LOOP_PATHS, fs.LOOP_FADES, sh.LOOP_SEED, r, n0) + nz
        b = faderef.bound(xw, Fs, fs.LOOP_PATHS, fs.LOOP_FADES, sh.LOOP_SEED, r, np.abs(nz))
        _check("u8", heard[k, r], y[block:], b[block:], ("loop", k, r))
        g = np.abs(faderef.gain(faderef.table(Fs, sh.LOOP_SEED, fs.LOOP_FADES[r]), n0 + block + np.arange(block, dtype=np.int64)))
        print(f"block {k}, receiver {r}: |g| of its far path from {g.min():.3f} to {g.max():.3f}")


# ---------------------------------------------------------------- 8. the command-line tool

@pytest.mark.parametrize("in_fmt,out_fmt", [("u8", "cf32"), ("cf32", "u8")])
def test_cli_with_fades_equals_the_binding(built_lib, tmp_path, in_fmt, out_fmt):
    import pirip_amd
    Fs, start = 240000, 2 ** 32 - 700
    paths, fades = fs.cut_paths(Fs)
    x, _ = sh.inputs(Fs, in_fmt, n=fs.CUT_N, ntx=2, seed=62)
    names = [str(tmp_path / f"{d}{i}") for d in ("in", "out") for i in range(2)]
    x[0].tofile(names[0])
    x[1].tofile(names[1])
    cmd = [os.path.join(ms.BIN, "air_channels"), "--fs", str(Fs), "--in-format", in_fmt, "--out-format", out_fmt, "--sigma", "0.05,0.08", "--seed", "9",
           "--block", "1000", "--start", str(start), "--max-slip", str(fs.CUT_SLIP), "-q"]
    for rx, tx, g, d, f, q in paths:
        cmd += ["--path", f"{rx},{tx},{g:.9g},{d},{f}" + (f",{q}" if q else "")]
    for path, hz, k, key in fades:
        cmd += ["--fade", f"{path},{int(round(hz * 1000))},{k:.9g}" + (f",{key}" if key else "")]
    p = subprocess.run(cmd + names[:2] + ["--"] + names[2:], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    air = pirip_amd.HipAir(Fs, paths, 2, 2, sigma=[0.05, 0.08], seed=9, in_format=_fmt(in_fmt), out_format=_fmt(out_fmt), max_slip=fs.CUT_SLIP, fades=fades)
    air.reset(start)
    want = _run(air, x, [fs.CUT_N])
    for r in range(2):
        got = np.fromfile(names[2 + r], dtype=np.uint8)
        assert got.size == fs.CUT_N * fs.BS[out_fmt] and np.array_equal(got, want[r]), r
    # a fade on a path that is not there: a handle that cannot be made
    bad = subprocess.run(cmd + ["--fade", "9,1000,0"] + names[:2] + ["--"] + names[2:], capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"channel" in bad.stderr
