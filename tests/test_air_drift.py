"""include/pirip_hip.h section O, drift: paths on sample clocks that disagree (pirip_hip_air_create_ex, pirip_amd.HipAir(max_slip=...)),
on the device.

Contract 1: every complex-float component within driftref.bound -- airref.bound with Lambda max |x| for a drifting path's |x| and
16 e Lambda |a_p| max |x| more, derived in DESIGN.md 4.15a -- of the float64 statement (tests/driftref.py) on the library's own table; u8
bytes within one level of the quantised model and different from it only inside airref.tie_window of that bound. Contract 2, bit for
bit: any cutting into calls equals one shot, n0 equals n0 + k Fs without noise, a handle of pirip_hip_air_create_ex without a clock
offset equals pirip_hip_air_create's, a receiver does not depend on another receiver's drifting paths. Contract 3: the slip budget --
the call that reaches max_slip is taken, the next sample is refused and nothing happened. Contract 4: the demodulator tracks a clock
300 ppm off through the channel, and terminal and repeater find each other over a medium whose two ends run on clocks 40 ppm apart.
tests/test_air_drift_cpu.py shows on the model alone that the inputs used here reach what they claim."""
import os
import subprocess

import numpy as np
import pytest

import airref
import airshapes as sh
import driftref
import driftshapes as ds
import muxshapes as ms
import sigutil
from test_air import BAD_ARG, CANARY, UNSUPPORTED, _check, _fmt, _run

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 7. the model

CASES = [(Fs, i, o) for Fs in ds.FSS for i, o in ds.FORMATS]


@pytest.mark.parametrize("Fs,in_fmt,out_fmt", CASES, ids=[f"{Fs}-{i}-{o}" for Fs, i, o in CASES])
def test_drift_matches_float64(built_lib, Fs, in_fmt, out_fmt):
    """two receivers that mix static and drifting paths (+-1, +-300000, +-10^6 ppb) of both transmitters, in two calls, without and with
    noise, from the clock ages of driftshapes.RUNS: S steps inside a tile, on a tile's first sample, on the second call's first sample, and
    the last run ends on |S| = max_slip = 2^20 - 4096 - 7"""
    import pirip_amd
    worst = 0.0
    for max_slip in (ds.SLIP_SMALL, ds.SLIP_LARGE):
        x, paths = ds.inputs(Fs, in_fmt, max_slip)
        xw = airref.widen(x, ds.FMT[in_fmt])
        air = pirip_amd.HipAir(Fs, paths, ds.NTX, ds.NRX, seed=ds.SEED, in_format=_fmt(in_fmt), out_format=_fmt(out_fmt), max_slip=max_slip)
        assert air.max_delay == max(p[3] for p in paths) and air.drift()[0] == max_slip
        for k, (_, age, n0) in enumerate(r for r in ds.RUNS if r[0] == max_slip):
            clean = [driftref.signal(xw, Fs, paths, r, n0, age0=age) for r in range(ds.NRX)]
            for sigma in (None, ds.SIGMA):
                air.set_sigma(sigma)
                air.reset(n0, age=age)
                left = air.drift()[1]
                assert left == driftref.samples_left(paths, max_slip, age)
                rows = _run(air, x, ds.CALLS, pad=k % 2)
                assert air.drift()[1] == left - ds.N
                for r in range(ds.NRX):
                    s = 0.0 if sigma is None else sigma[r]
                    nz = airref.noise(ds.SEED, r, n0, ds.N, s)
                    b = driftref.bound(xw, paths, r, np.abs(nz)) if s else driftref.bound(xw, paths, r)
                    fig = _check(out_fmt, rows[r], clean[r] + nz, b, (Fs, in_fmt, out_fmt, max_slip, age, n0, s, r))
                    print(f"Fs {Fs} {in_fmt}->{out_fmt} max_slip {max_slip} age {age} n0 {n0} sigma {s} receiver {r}: "
                          + (f"largest error / bound {fig:.3f}" if out_fmt == "cf32" else f"share of components inside a tie window {fig:.2e}"))
                    if out_fmt == "cf32":
                        worst = max(worst, fig)
        air.close()
    if out_fmt == "cf32":
        print(f"Fs {Fs} {in_fmt}->{out_fmt}: largest error / bound of the case {worst:.3f}")


# ---------------------------------------------------------------- 8. cutting

@pytest.mark.parametrize("in_fmt,out_fmt", ds.FORMATS, ids=[f"{i}-{o}" for i, o in ds.FORMATS])
def test_any_cutting_equals_one_shot_under_drift(built_lib, in_fmt, out_fmt):
    import pirip_amd
    Fs = 240000
    paths = ds.cut_paths(Fs)
    x, _ = sh.inputs(Fs, in_fmt, n=ds.CUT_N, ntx=2, seed=60)
    cuts = ds.CUTS + [ds.CUT_N - sum(ds.CUTS)]
    air = pirip_amd.HipAir(Fs, paths, 2, 2, sigma=[0.05, 0.08], seed=9, in_format=_fmt(in_fmt), out_format=_fmt(out_fmt), max_slip=ds.CUT_SLIP)
    air.reset(ds.CUT_START, age=ds.CUT_AGE)
    whole = _run(air, x, [ds.CUT_N])
    for pad in (0, 1):
        air.reset(ds.CUT_START, age=ds.CUT_AGE)
        assert np.array_equal(_run(air, x, cuts, pad=pad), whole), pad
    air.reset(ds.CUT_START, age=ds.CUT_AGE)
    assert np.array_equal(_run(air, x, [ds.CUT_N], pad=1), whole)
    air.reset(ds.CUT_START, age=ds.CUT_AGE)
    assert np.array_equal(_run(air, x, cuts[::-1]), whole)                   # the long call first
    # and it is the model's
    xw = airref.widen(x, ds.FMT[in_fmt])
    for r, s in enumerate((0.05, 0.08)):
        nz = airref.noise(9, r, ds.CUT_START, ds.CUT_N, s)
        _check(out_fmt, whole[r], driftref.signal(xw, Fs, paths, r, ds.CUT_START, age0=ds.CUT_AGE) + nz, driftref.bound(xw, paths, r, np.abs(nz)),
               (in_fmt, out_fmt, r))
    # without noise the start only counts modulo Fs; the clock age counts
    air.set_sigma(None)
    air.reset(ds.CUT_START, age=ds.CUT_AGE)
    quiet = _run(air, x, cuts)
    air.reset(ds.CUT_START + 3 * Fs, age=ds.CUT_AGE)
    assert np.array_equal(_run(air, x, [ds.CUT_N]), quiet)
    air.reset(ds.CUT_START, age=ds.CUT_AGE + 1)
    assert not np.array_equal(_run(air, x, [ds.CUT_N]), quiet)
    assert not np.array_equal(quiet, whole)


# ---------------------------------------------------------------- 9. no change

@pytest.mark.parametrize("in_fmt,out_fmt", ds.FORMATS, ids=[f"{i}-{o}" for i, o in ds.FORMATS])
def test_without_a_clock_offset_nothing_changes(built_lib, in_fmt, out_fmt):
    """pirip_hip_air_create_ex with every q = 0 gives pirip_hip_air_create's bytes; and a receiver's bytes do not depend on another
    receiver's drifting paths, which put the whole handle on the other kernel (canaries round every row)"""
    import pirip_amd
    Fs = 240000
    x, paths = sh.inputs(Fs, in_fmt)
    kw = dict(sigma=sh.SIGMA, seed=sh.SEED, in_format=_fmt(in_fmt), out_format=_fmt(out_fmt))
    n0 = Fs - 5
    plain = pirip_amd.HipAir(Fs, paths, sh.NTX, sh.NRX, **kw)
    plain.reset(n0)
    want = _run(plain, x, sh.CALLS)
    ex = pirip_amd.HipAir(Fs, [p + (0,) for p in paths], sh.NTX, sh.NRX, max_slip=5, **kw)
    assert ex.drift()[0] == 5
    ex.reset(n0, age=12345)
    assert np.array_equal(_run(ex, x, sh.CALLS, pad=1), want)
    # receiver 0 of airshapes' layout has no path: give it drifting ones
    mixed = pirip_amd.HipAir(Fs, [p + (0,) for p in paths] + [(0, 0, 0.1, 40, 77, 300000), (0, 1, -0.1, 9, 0, -1000000)], sh.NTX, sh.NRX, max_slip=20, **kw)
    mixed.reset(n0, age=2000)
    got = _run(mixed, x, sh.CALLS)
    assert np.array_equal(got[1:], want[1:]) and not np.array_equal(got[0], want[0])


# ---------------------------------------------------------------- 10. the budget

@pytest.mark.parametrize("q", [10 ** 6, -10 ** 6])
def test_slip_budget(built_lib, q):
    """max_slip 2 at +-10^6 ppb: clock ages 0 .. 2999 (fast) or 0 .. 2000 (slow) are taken, the next one is refused and nothing happened"""
    import torch
    import pirip_amd
    total = 3000 if q > 0 else 2001
    paths = [(0, 0, 1.0, 10, 0, q)]
    assert driftref.samples_left(paths, 2, 0) == total
    air = pirip_amd.HipAir(240000, paths, 1, 1, max_slip=2)
    assert air.drift() == (2, total)
    d_in = torch.randint(0, 256, (8192,), dtype=torch.uint8, device="cuda")
    d_out = torch.full((8192,), CANARY, dtype=torch.uint8, device="cuda")
    with pytest.raises(pirip_amd.PiripError, match=rf"\({UNSUPPORTED}\)"):
        air.push(d_in, 8192, total + 1, d_out, 8192)                             # one sample too many, from the start
    assert air.drift() == (2, total)
    air.push(d_in, 8192, 1000, d_out, 8192)
    assert air.drift() == (2, total - 1000)
    air.push(d_in.data_ptr() + 2000, 8192, 1, d_out.data_ptr() + 2000, 8192)
    assert air.drift() == (2, total - 1001)
    torch.cuda.synchronize()
    before = d_out.cpu().numpy().copy()
    with pytest.raises(pirip_amd.PiripError, match=rf"\({UNSUPPORTED}\)"):
        air.push(d_in, 8192, total - 1000, d_out, 8192)
    torch.cuda.synchronize()
    assert air.drift() == (2, total - 1001) and np.array_equal(d_out.cpu().numpy(), before)     # nothing enqueued, no state changed
    air.push(d_in, 8192, total - 1001, d_out, 8192)                              # the call whose last sample reaches |S| = max_slip
    assert air.drift() == (2, 0)
    with pytest.raises(pirip_amd.PiripError, match=rf"\({UNSUPPORTED}\)"):
        air.push(d_in, 8192, 1, d_out, 8192)
    assert air.drift() == (2, 0)
    # the accepted run is the model's, its last sample at |S| = 2
    air.reset(0)
    assert air.drift() == (2, total)
    x = d_in.cpu().numpy()[:total * 2].reshape(1, total, 2)
    row = _run(air, x, [1000, total - 1000])[0]
    xw = airref.widen(x, airref.U8)
    assert abs(int(driftref.slip(total - 1, q)[0])) == 2
    _check("u8", row, driftref.signal(xw, 240000, paths, 0, 0), driftref.bound(xw, paths, 0), ("budget", q))
    assert air.drift() == (2, 0)
    # reset_drift: an age inside the budget, the last one, and one past it
    air.reset(7, age=total - 1)
    assert air.drift() == (2, 1)
    with pytest.raises(pirip_amd.PiripError, match=rf"\({UNSUPPORTED}\)"):
        air.reset(7, age=total)
    with pytest.raises(pirip_amd.PiripError, match=rf"\({BAD_ARG}\)"):
        air.reset(7, age=-1)
    assert air.drift() == (2, 1)
    air.push(d_in, 8192, 1, d_out, 8192)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 11. demodulation on the device

def test_demodulator_tracks_a_clock_300_ppm_off_through_the_channel(built_lib, oracle):
    """tests/test_air_drift_cpu.py's signal through HipAir (u8 -> u8, one receiver on a fast clock, one on a slow one) into HipDemod: the
    transmitted test bits without an error after the first frame, two short frames on the fast clock and two long ones on the slow one"""
    import pirip_amd
    c = sigutil.CFG1
    u8, _ = ds.clock_input(oracle)
    air = pirip_amd.HipAir(c["Fs"], ds.clock_paths(), 1, 2, max_slip=ds.CLOCK_SLIP)
    n = u8.shape[0]
    rows = _run(air, u8[None], [n // 2 + 11, n - n // 2 - 11]).reshape(2, n, 2)
    for r, name in enumerate(("fast", "slow")):
        h = pirip_amd.HipDemod(c["Fs"], c["Rs"], c["M"], P=c["P"], est_min=c["est_min"], est_max=c["est_max"], nstreams=1)
        rh = h.demod_host(np.ascontiguousarray(rows[r]))
        nin = rh["stats"][:, 6]
        short, long_ = int((nin < h.N).sum()), int((nin > h.N).sum())
        res = oracle.put_test_bits(rh["bits"][1:].reshape(-1))
        print(f"{name}: {rh['nframes']} frames, {short} short, {long_} long, {res['bits']} test bits, {res['errors']} errors")
        assert rh["nframes"] >= 35 and res["bits"] > 1500 and res["errors"] == 0
        assert (short if r == 0 else long_) >= 2


# ---------------------------------------------------------------- 12. the shared-medium loop on two clocks

@pytest.fixture(scope="module")
def medium(built_lib):
    """tests/test_air.py's medium with far paths whose clocks run 20000 ppb fast one way and 20000 ppb slow the other; the leaks stay
    static"""
    import torch
    import pirip_amd
    from test_ping import LOOP_CALLS, _Repeater, _Terminal
    term, rep = _Terminal(), _Repeater()
    block, blk, K = term.block, term.block * 2, LOOP_CALLS
    assert rep.block == block and sh.FAR["delay"] < block
    air = pirip_amd.HipAir(ms.LOOP["Fs"], ds.LOOP_PATHS, 2, 2, sigma=sh.LOOP_SIGMA, seed=sh.LOOP_SEED, max_slip=ds.LOOP_SLIP)
    left = air.drift()[1]
    assert left >= K * block, "the loop outlasts its slip budget"
    sent = torch.full((K + 1, 2, blk), 128, dtype=torch.uint8, device="cuda")
    heard = torch.zeros((K, 2, blk), dtype=torch.uint8, device="cuda")
    for k in range(K):
        air.push(sent[k], blk, block, heard[k], blk)
        term.ping.push(heard[k, 0], blk, sent[k + 1, 0], blk)
        rep.rpt.push(heard[k, 1], blk, sent[k + 1, 1], blk)
    torch.cuda.synchronize()
    assert air.drift()[1] == left - K * block
    return dict(term=term, rep=rep, air=air, sent=sent, heard=heard, logs=[term.ping.log(c) for c in range(4)], ping=term.ping.counters(),
                rpt=rep.rpt.counters())


def test_shared_medium_loop_on_two_clocks(medium):
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


def test_what_each_end_heard_on_two_clocks_is_the_models(medium):
    """the last busy block and the one before it, both receivers: the channel's bytes are the float64 statement's at that clock age"""
    sent, heard = medium["sent"].cpu().numpy(), medium["heard"].cpu().numpy()
    block = medium["term"].block
    busy = [k for k in range(1, heard.shape[0]) if (sent[k - 1:k + 1, 1] != 128).any() and (sent[k - 1:k + 1, 0] != 128).any()]
    k = busy[-1] if busy else max(k for k in range(1, heard.shape[0]) if (sent[k] != 128).any())
    x = np.concatenate([sent[k - 1], sent[k]], axis=1).reshape(2, 2 * block, 2)
    xw = airref.widen(x, airref.U8)
    n0 = (k - 1) * block
    assert sh.FAR["delay"] + 7 + ds.LOOP_SLIP < block            # no lag reaches from the second block past the first
    print(f"block {k}: S = {int(driftref.slip(n0 + 2 * block - 1, ds.LOOP_PPB)[0])} and {int(driftref.slip(n0 + 2 * block - 1, -ds.LOOP_PPB)[0])} on its last sample")
    for r in range(2):
        nz = airref.noise(sh.LOOP_SEED, r, n0, 2 * block, sh.LOOP_SIGMA)
        # (the model takes block k - 1 for the first since a reset, at the clock age it had: the second block sees no further back)
        y = driftref.signal(xw, ms.LOOP["Fs"], ds.LOOP_PATHS, r, n0, age0=n0) + nz
        b = driftref.bound(xw, ds.LOOP_PATHS, r, np.abs(nz))
        _check("u8", heard[k, r], y[block:], b[block:], ("loop", k, r))


# ---------------------------------------------------------------- 13. the command-line tool

@pytest.mark.parametrize("in_fmt,out_fmt", [("u8", "cf32"), ("cf32", "u8")])
def test_cli_with_clock_offsets_equals_the_binding(built_lib, tmp_path, in_fmt, out_fmt):
    import pirip_amd
    Fs, start = 240000, 2 ** 31 + 3
    paths = ds.cut_paths(Fs)
    x, _ = sh.inputs(Fs, in_fmt, n=ds.CUT_N, ntx=2, seed=62)
    names = [str(tmp_path / f"{d}{i}") for d in ("in", "out") for i in range(2)]
    x[0].tofile(names[0])
    x[1].tofile(names[1])
    cmd = [os.path.join(ms.BIN, "air_channels"), "--fs", str(Fs), "--in-format", in_fmt, "--out-format", out_fmt, "--sigma", "0.05,0.08", "--seed", "9",
           "--block", "1000", "--start", str(start), "--max-slip", str(ds.CUT_SLIP), "-q"]
    for rx, tx, g, d, f, q in paths:
        cmd += ["--path", f"{rx},{tx},{g:.9g},{d},{f}" + (f",{q}" if q else "")]
    p = subprocess.run(cmd + names[:2] + ["--"] + names[2:], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    air = pirip_amd.HipAir(Fs, paths, 2, 2, sigma=[0.05, 0.08], seed=9, in_format=_fmt(in_fmt), out_format=_fmt(out_fmt), max_slip=ds.CUT_SLIP)
    air.reset(start)
    want = _run(air, x, [ds.CUT_N])
    for r in range(2):
        got = np.fromfile(names[2 + r], dtype=np.uint8)
        assert got.size == ds.CUT_N * ds.BS[out_fmt] and np.array_equal(got, want[r]), r
    # a clock offset without --max-slip: a handle that cannot be made
    at = cmd.index("--max-slip")
    bad = subprocess.run(cmd[:at] + cmd[at + 2:] + names[:2] + ["--"] + names[2:], capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"channel" in bad.stderr
