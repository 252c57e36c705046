"""include/pirip_hip.h section N: the ping terminal (pirip_hip_ping_*, pirip_amd.HipPing), ping_channels and rtl_fsk_channels -L.

Every comparison is exact unless it says otherwise. The log and the schedule come from the host model tests/pingref.py, which
tests/test_ping_cpu.py pins to the framer's own test frames and whose tables it shows to reach every corner; the IQ must be what a fresh
HipTxStream makes when the host sends it the model's records call by call (section M's contract); the log's columns must be those of
rtl_fsk -L on the same samples. The closed loop runs the terminal against the streaming repeater, each fed the other's previous block."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import muxshapes as ms
import pingref
import rptref
import sigutil

pytestmark = pytest.mark.gpu

CANARY = 0xA5
BAD_ARG, UNSUPPORTED = -1, -6
LOOP_S, LOOP_GAP, LOOP_CALLS = 100, 64, 90
ROUTE = [1, 0, 3, 2]
FIRST = [2, 3, 4, 5]


def _want():
    import pirip_amd
    return pirip_amd.testframe_payload(8 * pingref.KB)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- 1. the records path

def _shape_rx(nrx):
    """a streaming receiver that only tells the logger its shape (channels, frame size, N = pingref.N0); it is never run"""
    import pirip_amd
    dem = pirip_amd.HipDemod(40000, 1000, 2, P=10, est_min=500, est_max=20000, nstreams=nrx)
    ld = pirip_amd.HipLdpc(ms.CODE, 2, nstreams=nrx)
    return dem, ld, pirip_amd.HipRx(dem, ldpc=ld, block=8000)


def _push_calls(ping, calls):
    """calls of pingref's rows through push_records, staged with slots behind a channel's count that would be logged, were they read"""
    import torch
    nrx, kb = len(calls[0]), pingref.KB
    keep = []
    for rows in calls:
        w = max([len(r[0]) for r in rows] + [1])
        st = np.full((nrx, w), pingref.SYNC | pingref.BITS, np.uint8)
        pl = np.full((nrx, w, kb), 0x5A, np.uint8)
        info = np.full((nrx, w, pingref.INFO), 77, np.int32)
        stats = np.full((nrx, w, pingref.STATS), 7777.0, np.float32)
        nc = np.zeros(nrx, np.int32)
        for c, (a, b, i, s) in enumerate(rows):
            n = len(a)
            st[c, :n], pl[c, :n], info[c, :n], stats[c, :n], nc[c] = a, b, i, s, n
        d = [torch.from_numpy(x).cuda() for x in (st, pl, info, stats, nc)]
        keep.append(d)
        ping.push_records(d[0], d[1], d[2], d[3], ncalls=d[4])
    torch.cuda.synchronize()
    return keep


def _check_log(ping, m):
    got = ping.counters()
    for k, v in m.counters().items():
        assert np.array_equal(got[k], v), (k, got[k], v)
    for c in range(m.nrx):
        log = ping.log(c)
        assert log.dtype == pingref.ENTRY and _same(log, m.log(c)), (c, log, m.log(c))
    return got


def test_records_path_equals_the_model(built_lib):
    """push_records on a logger-only handle of three channels. The frame's size is not part of the configuration, so the handle takes
    its shape from a streaming receiver, which is never run: every row comes from the caller."""
    import pirip_amd
    want = _want()
    dem, ld, rx = _shape_rx(3)
    ping = pirip_amd.HipPing(rx=rx, filter=pingref.FILT, log_entries=pingref.LOG_ENTRIES)
    assert (ping.nrx, ping.nchan, ping.nin0, ping.data_bytes, ping.info.has_rx) == (3, 0, pingref.N0, pingref.KB, 1)
    calls = pingref.log_calls(want)
    _push_calls(ping, calls)
    got = _check_log(ping, pingref.run_log(calls, want))
    assert got["filtered"].all() and got["crc_fail"].any() and got["lost"].any() and got["bit_errors"].any()
    assert _same(ping.log(0, 3), ping.log(0)[-3:]) and len(ping.log(0, 0)) == 0
    # one call of 4096 rows behind them, on the ring and on one that holds them all
    rng = np.random.default_rng(8)
    big = [[pingref._rows(rng, n, want) for n in (4096, 4095, 1)]]
    _push_calls(ping, big)
    _check_log(ping, pingref.run_log(calls + big, want))
    wide = pirip_amd.HipPing(rx=rx, filter=pingref.FILT, log_entries=5000)
    _push_calls(wide, calls + big)
    m = pingref.run_log(calls + big, want, log_entries=5000)
    _check_log(wide, m)
    assert m.c["frames"][0] > 1000 and not m.c["lost"].any()
    # the same rows cut into other calls: only call and row differ
    for seed in (3, 4):
        wide.reset()
        assert not any(v.any() for v in wide.counters().values()) and len(wide.log(0)) == 0
        _push_calls(wide, pingref.recut(calls + big, seed))
        got = wide.counters()
        for k, v in m.counters().items():
            assert np.array_equal(got[k], v), k
        for c in range(3):
            assert pingref.same_but_call_and_row(wide.log(c), m.log(c)), c
        assert wide.log(0)["call"].tolist() != m.log(0)["call"].tolist()


# ---------------------------------------------------------------- 2. the scheduler

def _tx_side(M, queue_syms, S=LOOP_S):
    import pirip_amd
    lp = ms.LOOP
    tx = pirip_amd.HipTx(ms.CODE, lp["mFs"], lp["Rs"], M, nstreams=4, f1=lp["f1"], shift=lp["shift"], gap=LOOP_GAP)
    mux = pirip_amd.HipMux(lp["Fs"], lp["D"], lp["offsets"], gains=ms.LOOP_GAINS)
    block = S * lp["D"] * tx.Ts
    return tx, mux, block, pirip_amd.HipTxStream(tx, mux, block, queue_syms)


def _host_driven(tx, mux, block, queue_syms, offered, rl):
    """a fresh HipTxStream of the same configuration, sent the model's records call by call -> IQ"""
    import torch
    import pirip_amd
    txs = pirip_amd.HipTxStream(tx, mux, block, queue_syms)
    K, P = len(offered), max(len(r) for per in offered for r in per)
    stage, nrec = np.full((K, 4, P, rl), 3, np.uint8), np.zeros((K, 4), np.int32)
    for n, per in enumerate(offered):
        for t, r in enumerate(per):
            stage[n, t, :len(r)], nrec[n, t] = r, len(r)
    d_stage, d_nrec = torch.from_numpy(stage).cuda(), torch.from_numpy(nrec).cuda()
    out = torch.zeros(K * block * 2, dtype=torch.uint8, device="cuda")
    for n in range(K):
        txs.send(d_stage[n].data_ptr(), P * rl, P, d_nrec=d_nrec[n].data_ptr())
        txs.process(out.data_ptr() + n * block * 2, block * 2)
    torch.cuda.synchronize()
    assert not txs.counters()["refused"].any()
    return out


CASES = [(n, M) for M in (2, 4) for n in ("staggered", "cutoff", "tight")]


@pytest.mark.parametrize("name,M", CASES, ids=["%s-M%d" % c for c in CASES])
def test_scheduler_equals_the_model_and_a_host_driven_transmitter(built_lib, name, M):
    import torch
    import pirip_amd
    pre, frame = (50, 544) if M == 2 else (100, 272)
    s = {x["name"]: x for x in pingref.schedules(pre, frame, LOOP_GAP)}[name]
    tx, mux, block, txs = _tx_side(M, s["queue_syms"])
    assert (tx.preamble_syms, tx.frame_syms, tx.data_bytes) == (pre, frame, pingref.KB)
    ping = pirip_amd.HipPing(tx=tx, txs=txs, nrx=1, source=1, filter=1, frames=3, seq=True, period=s["period"], first_call=s["first_call"],
                             max_bursts=s["max_bursts"], log_entries=4)
    burst = pingref.burst_records(_want(), 3, 1, True)
    offered, m = pingref.run_schedule(s, burst)
    K, blk, rl = s["calls"], block * 2, 1 + pingref.KB
    rt = sigutil.hip_runtime()
    p_rec, stride, p_n = ping.offered()
    assert stride == 4 * rl
    out = torch.full((K * blk + 64,), CANARY, dtype=torch.uint8, device="cuda")
    off = torch.full((K, 4, 4, rl), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((K, 4), -7, dtype=torch.int32, device="cuda")
    none = [torch.zeros(16, dtype=dt, device="cuda") for dt in (torch.uint8, torch.uint8, torch.int32, torch.float32)]
    for n in range(K):
        ping.push_records(none[0], none[1], none[2], none[3], out=out.data_ptr() + 32 + n * blk, out_stride=blk, max_calls=0, status_stride=0,
                          payload_stride=0, info_stride=0, stats_stride=0)
        sigutil.d2d(rt, off[n].data_ptr(), p_rec, 4 * stride)
        sigutil.d2d(rt, cnt[n].data_ptr(), p_n, 4 * 4)
    torch.cuda.synchronize()
    assert (out[:32] == CANARY).all() and (out[32 + K * blk:] == CANARY).all()
    off, cnt = off.cpu().numpy(), cnt.cpu().numpy()
    for n, per in enumerate(offered):
        assert cnt[n].tolist() == [len(r) for r in per], (name, n)
        for t, r in enumerate(per):
            assert np.array_equal(off[n, t, :len(r)], r), (name, n, t)
    got = ping.counters()
    for k, v in m.c.items():
        assert np.array_equal(got[k], v), (k, got[k], v)
    assert not got["frames"].any()
    c = txs.counters()
    assert not c["refused"].any() and np.array_equal(c["queued"], np.array(m.queued))
    if name == "tight":
        assert (got["skipped"] > 0).all()
    iq = out[32:32 + K * blk]
    ref = _host_driven(tx, mux, block, s["queue_syms"], offered, rl)
    assert torch.equal(iq, ref), (name, M, int((iq != ref).sum()))
    assert (iq != 128).any()


# ---------------------------------------------------------------- 3. rtl_fsk -L

LINE = re.compile(r"Rx frame src: (0x[0-9a-f]{2}) seq: ( *\d+) S: (\S+) N: (\S+) SNR: ( *\S+) dB t_rx: (\S+) s")


def test_log_equals_rtl_fsk_L(built_lib, tmp_path):
    """One burst of three test frames at modem rate through the rtl_fsk CLI and through HipRx -> HipPing in blocks of another size: the
    src, seq, S, N and t_rx columns are string-equal under the CLI's format strings; the SNR column, whose operands are the same floats,
    is within 0.01 dB (the hosts' log10)."""
    import torch
    import pirip_amd
    Fs, Rs, block, nsym = 40000, 1000, 8000, 2600                  # 200 symbols of lead, the burst, 718 of tail: 13 blocks
    tx = pirip_amd.HipTx(ms.CODE, Fs, Rs, 2, nstreams=1, f1=1000, shift=2000, lead=200, gap=0)
    rec = torch.from_numpy(pingref.burst_records(_want(), 3, 1, True)).cuda()
    u8 = torch.zeros(nsym * tx.Ts * 2, dtype=torch.uint8, device="cuda")
    tx.records_to_iq(rec.data_ptr(), rec.numel(), 4, nsym, u8.data_ptr(), u8.numel())
    torch.cuda.synchronize()
    assert u8.numel() % (block * 2) == 0
    src = str(tmp_path / "burst.iq")
    u8.cpu().numpy().tofile(src)
    p = subprocess.run([os.path.join(ms.BIN, "rtl_fsk"), "-i", src, "-s", str(Fs), "-a", str(Fs), "-r", str(Rs), "--code", ms.CODE, "-L", "-q",
                        str(tmp_path / "payloads")], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    cli = [LINE.search(ln).groups() for ln in p.stderr.decode().splitlines() if "Rx frame" in ln]
    # the modem settings rtl_fsk derives: P = 10 of Ts = 40, the estimator from Rs / 2 to Fs / 2, bytes read as b / 127.5 - 1
    dem = pirip_amd.HipDemod(Fs, Rs, 2, P=10, est_min=Rs // 2, est_max=Fs // 2, in_format=pirip_amd.IN_CU8_CSDR, nstreams=1)
    ld = pirip_amd.HipLdpc(ms.CODE, 2, nstreams=1)
    rx = pirip_amd.HipRx(dem, ldpc=ld, block=block)
    ping = pirip_amd.HipPing(rx=rx, log_entries=16)
    for k in range(u8.numel() // (block * 2)):
        ping.push(u8.data_ptr() + k * block * 2, block * 2)
    log = ping.log(0)
    assert len(cli) == 3 and len(log) == 3
    for e, (s_src, s_seq, s_S, s_N, s_snr, s_t) in zip(log, cli):
        S, N = float(e["S"]), float(e["N"])
        assert ("0x%02x" % e["source"], "%3d" % e["seq"], "%e" % S, "%e" % N, "%.4f" % (int(e["t_samples"]) / float(Fs))) == \
               (s_src, s_seq, s_S, s_N, s_t)
        assert abs(10.0 * math.log10(S / (N + 1e-30) + 1e-30) - float(s_snr)) <= 0.01
    assert log["source"].tolist() == [1, 1, 1] and log["seq"].tolist() == [1, 2, 3] and not log["ecdd"].any()
    assert ping.counters()["frames"].tolist() == [3]


# ---------------------------------------------------------------- 4 - 6. the closed loop (tests/muxshapes.py's LOOP)

class _Terminal:
    """HipPing(rx=HipRx(chan=...), tx, txs) of the LOOP shapes; the handles it borrows live as long as it does"""

    def __init__(self, log_entries=16):
        import pirip_amd
        from test_mux import _rx_handles
        lp = ms.LOOP
        burst = 50 + lp["nframes"] * 544 + LOOP_GAP
        self.tx, self.mux, self.block, self.txs = _tx_side(lp["M"], burst)
        self.dem, self.ld, self.ch = _rx_handles()
        self.rx = pirip_amd.HipRx(self.dem, ldpc=self.ld, chan=self.ch, block=self.block)
        self.ping = pirip_amd.HipPing(rx=self.rx, tx=self.tx, txs=self.txs, source=1, filter=1, frames=lp["nframes"], seq=True, period=1,
                                      first_call=FIRST, max_bursts=1, log_entries=log_entries)
        assert self.ping.rx_rows == self.rx.max_frames and self.ping.nin0 == self.dem.N and self.ping.nchan == 4


class _Repeater:
    """tests/test_repeater_stream.py's arrangement: source 2, filter 2, route [1, 0, 3, 2], hold-off 1"""

    def __init__(self):
        import pirip_amd
        from test_mux import _rx_handles
        lp = ms.LOOP
        burst = 50 + lp["nframes"] * 544 + LOOP_GAP
        self.tx, self.mux, self.block, self.txs = _tx_side(lp["M"], burst)
        self.dem, self.ld, self.ch = _rx_handles()
        self.rx = pirip_amd.HipRx(self.dem, ldpc=self.ld, chan=self.ch, block=self.block)
        self.rpt = pirip_amd.HipRepeater(self.tx, self.txs, ROUTE, 2, filter=2, holdoff=1, max_burst=lp["nframes"], pending=lp["nframes"] + 1,
                                         rx=self.rx)


def _run_loop(term, rep, tbits=None, K=LOOP_CALLS):
    """the two handles step block by block, each fed the other's previous output (silence first) -> dict of the terminal's and the
    repeater's blocks and copies of the terminal's records() of every call"""
    import torch
    rt = sigutil.hip_runtime()
    blk = term.block * 2
    R, kb = term.ping.rx_rows, pingref.KB
    silence = torch.full((blk,), 128, dtype=torch.uint8, device="cuda")
    t_out = torch.zeros((K, blk), dtype=torch.uint8, device="cuda")
    r_out = torch.zeros((K, blk), dtype=torch.uint8, device="cuda")
    st = torch.zeros((K, 4, R), dtype=torch.uint8, device="cuda")
    pl = torch.zeros((K, 4, R, kb), dtype=torch.uint8, device="cuda")
    info = torch.zeros((K, 4, R, 10), dtype=torch.int32, device="cuda")
    stats = torch.zeros((K, 4, R, 10), dtype=torch.float32, device="cuda")
    nfr = torch.zeros((K, 4), dtype=torch.int32, device="cuda")
    for k in range(K):
        term.ping.push(r_out[k - 1] if k else silence, blk, t_out[k], blk)
        r = term.ping.records()
        assert (r["status_stride"], r["payload_stride"], r["info_stride"], r["stats_stride"]) == (R, R * kb, R * 10, R * 10)
        if tbits is not None:
            tbits.push_records(r["status"], r["payload"], r["info"], ncalls=r["nframes"], max_calls=R, status_stride=R, payload_stride=R * kb,
                               info_stride=R * 10)
        sigutil.d2d(rt, st[k].data_ptr(), r["status"], 4 * R)
        sigutil.d2d(rt, pl[k].data_ptr(), r["payload"], 4 * R * kb)
        sigutil.d2d(rt, info[k].data_ptr(), r["info"], 4 * R * 10 * 4)
        sigutil.d2d(rt, stats[k].data_ptr(), r["stats"], 4 * R * 10 * 4)
        sigutil.d2d(rt, nfr[k].data_ptr(), r["nframes"], 4 * 4)
        rep.rpt.push(t_out[k - 1] if k else silence, blk, r_out[k], blk)
    torch.cuda.synchronize()
    return dict(t_out=t_out, r_out=r_out, seen=[x.cpu().numpy() for x in (st, pl, info, stats, nfr)], logs=[term.ping.log(c) for c in range(4)],
                counters=term.ping.counters())


@pytest.fixture(scope="module")
def loop(built_lib):
    import pirip_amd
    term, rep = _Terminal(), _Repeater()
    tb = pirip_amd.HipTestBits(nstreams=4)
    tb.set_payload(pingref.KB)
    out = _run_loop(term, rep, tbits=tb)
    out.update(term=term, rep=rep, tb=tb.record_counters(), rpt=rep.rpt.counters())
    return out


def test_closed_loop_every_frame_comes_back_and_is_logged(loop):
    nfr = ms.LOOP["nframes"]
    c = loop["counters"]
    for ch in range(4):
        log = loop["logs"][ch]
        assert len(log) == nfr, (ch, log)
        assert log["source"].tolist() == [2] * nfr and log["seq"].tolist() == [1, 2, 3] and not log["ecdd"].any()
        assert (np.diff(log["t_samples"]) > 0).all()
    assert np.array_equal(c["frames_sent"], c["frames"]) and c["frames"].tolist() == [nfr] * 4 and c["bursts_sent"].tolist() == [1] * 4
    assert not c["skipped"].any() and not c["lost"].any() and not c["filtered"].any() and not c["bit_errors"].any()
    assert loop["rpt"]["bursts_in"].tolist() == [1] * 4 and loop["rpt"]["bursts_out"].tolist() == [1] * 4
    # the log is the model's on the copies of records() taken each call
    term = loop["term"]
    st, pl, info, stats, nf = loop["seen"]
    m = pingref.Log(4, term.ping.nin0, 1, term.ping.log_entries, _want())
    for k in range(st.shape[0]):
        m.call([(st[k, ch, :nf[k, ch]], pl[k, ch, :nf[k, ch]], info[k, ch, :nf[k, ch]], stats[k, ch, :nf[k, ch]]) for ch in range(4)])
    for ch in range(4):
        assert _same(loop["logs"][ch], m.log(ch)), ch
    for k, v in m.counters().items():
        assert np.array_equal(c[k], v), k
    assert nf.sum(axis=0).min() > 20                                 # the clock ran over many rows
    # a counter chained on records() saw the same frames pass their CRC
    assert np.array_equal(loop["tb"]["crc_ok"], c["frames"])


def test_own_output_is_filtered(loop):
    import torch
    term = loop["term"]
    term.ping.reset()
    assert not any(v.any() for v in term.ping.counters().values())
    blk = term.block * 2
    sink = torch.zeros(blk, dtype=torch.uint8, device="cuda")
    for k in range(LOOP_CALLS):
        term.ping.push(loop["t_out"][k], blk, sink, blk)
    c = term.ping.counters()
    assert c["filtered"].tolist() == [ms.LOOP["nframes"]] * 4 and not c["frames"].any() and not c["lost"].any()
    assert all(len(term.ping.log(ch)) == 0 for ch in range(4))
    assert c["decoded"].min() >= ms.LOOP["nframes"]


def test_reset_repeats_the_first_run(loop):
    import torch
    term, rep = loop["term"], loop["rep"]
    term.ping.reset()
    rep.rpt.reset()
    again = _run_loop(term, rep)
    assert torch.equal(again["t_out"], loop["t_out"]) and torch.equal(again["r_out"], loop["r_out"])
    assert (loop["t_out"] != 128).any() and (loop["r_out"] != 128).any()
    for ch in range(4):
        assert _same(again["logs"][ch], loop["logs"][ch])
    assert all(np.array_equal(again["counters"][k], loop["counters"][k]) for k in loop["counters"])


# ---------------------------------------------------------------- 7. argument limits

def test_argument_limits_as_the_header_states_them(built_lib):
    import torch
    import pirip_amd
    pre, frame = 50, 544
    one = rptref.burst_cost(3, pre, frame, LOOP_GAP)
    tx, mux, block, txs = _tx_side(2, one, S=3)
    dem, ld, rx = _shape_rx(2)

    def fails(code, **kw):
        args = dict(tx=tx, txs=txs, nrx=2, source=1, filter=1, frames=3, period=1, log_entries=4)
        args.update(kw)
        with pytest.raises(pirip_amd.PiripError, match=rf"\({code}\)"):
            pirip_amd.HipPing(**args)

    fails(BAD_ARG, txs=None)                                         # one of tx / txs without the other
    fails(BAD_ARG, tx=None)
    fails(BAD_ARG, tx=None, txs=None)                                # nothing at all
    fails(BAD_ARG, rx=rx, nrx=3)                                     # not rx's channels
    fails(BAD_ARG, nrx=0)
    fails(BAD_ARG, source=256)
    fails(BAD_ARG, source=-1)
    fails(BAD_ARG, filter=256)
    fails(BAD_ARG, filter=-2)
    fails(BAD_ARG, frames=0)
    fails(BAD_ARG, frames=101)
    fails(BAD_ARG, frames=4)                                         # the queue holds a burst of three
    fails(BAD_ARG, period=0)
    fails(BAD_ARG, first_call=[0, 0, -1, 0])
    fails(BAD_ARG, max_bursts=-1)
    fails(BAD_ARG, log_entries=0)
    fails(BAD_ARG, nin0=-1)
    other = pirip_amd.HipTx(ms.CODE, ms.LOOP["mFs"], ms.LOOP["Rs"], 2, nstreams=4)
    fails(BAD_ARG, tx=other)                                         # txs was not created on this tx
    with pytest.raises(ValueError):
        pirip_amd.HipPing(tx=tx, txs=txs, nrx=1, first_call=[0, 0])
    blk = block * 2
    out = torch.zeros(blk, dtype=torch.uint8, device="cuda")
    both = pirip_amd.HipPing(rx=rx, tx=tx, txs=txs, frames=3, log_entries=4)
    sender = pirip_amd.HipPing(tx=tx, txs=txs, nrx=2, frames=3, log_entries=4, max_bursts=1, first_call=[9] * 4)
    logger = pirip_amd.HipPing(rx=rx, log_entries=4)
    assert (both.nrx, both.nchan, logger.nchan, sender.info.has_rx) == (2, 4, 0, 0)
    L = logger.L

    def push(h, ncalls, d_out, stats=True):
        w = max(ncalls, 1)
        st = torch.zeros((2, w), dtype=torch.uint8, device="cuda")
        pl = torch.zeros((2, w, pingref.KB), dtype=torch.uint8, device="cuda")
        info = torch.full((2, w, 10), -1, dtype=torch.int32, device="cuda")       # nothing decoded
        sts = torch.zeros((2, w, 10), dtype=torch.float32, device="cuda")
        rc = L.pirip_hip_ping_push_records(h.h, st.data_ptr(), ncalls, pl.data_ptr(), ncalls * pingref.KB, info.data_ptr(), ncalls * 10,
                                           sts.data_ptr() if stats else 0, ncalls * 10, 0, ncalls, d_out, blk, 0)
        torch.cuda.synchronize()
        return rc

    assert L.pirip_hip_ping_records(logger.h, *([None] * 9)) == BAD_ARG          # before the first call
    assert push(logger, 4097, 0) == UNSUPPORTED and push(logger, 4096, 0) == 0 and push(logger, 0, 0) == 0
    assert push(logger, 1, out.data_ptr()) == BAD_ARG                 # a logger has no output
    assert push(logger, 1, 0, stats=False) == BAD_ARG and push(logger, -1, 0) == BAD_ARG
    assert push(sender, 1, 0) == BAD_ARG and push(sender, 1, out.data_ptr()) == 0 and push(sender, 4097, out.data_ptr()) == UNSUPPORTED
    assert L.pirip_hip_ping_process(sender.h, out.data_ptr(), blk, 0) == BAD_ARG          # no rx
    assert L.pirip_hip_ping_push(sender.h, out.data_ptr(), blk, out.data_ptr(), blk, 0) == BAD_ARG
    assert L.pirip_hip_ping_push(logger.h, 0, blk, 0, 0, 0) == BAD_ARG             # no input
    assert L.pirip_hip_ping_process(logger.h, out.data_ptr(), blk, 0) == BAD_ARG    # a logger has no output
    assert L.pirip_hip_ping_process(both.h, 0, 0, 0) == BAD_ARG                     # a terminal needs one
    assert L.pirip_hip_ping_offered(logger.h, None, None, None) == BAD_ARG
    assert L.pirip_hip_ping_records(logger.h, *([None] * 9)) == 0
    got = C.c_int(-1)
    assert L.pirip_hip_ping_get_log(logger.h, 2, None, 0, C.byref(got)) == BAD_ARG and L.pirip_hip_ping_get_log(logger.h, -1, None, 0, None) == BAD_ARG
    assert L.pirip_hip_ping_get_log(logger.h, 0, None, 1, None) == BAD_ARG and L.pirip_hip_ping_get_log(logger.h, 0, None, -1, None) == BAD_ARG
    assert L.pirip_hip_ping_get_log(logger.h, 1, None, 0, C.byref(got)) == 0 and got.value == 0
    torch.cuda.synchronize()
    assert (out == 128).all()                                        # the one call that ran sent silence: nothing is due before call 9
    assert not any(v.any() for v in logger.counters().values()) and not any(v.any() for v in sender.counters().values())


# ---------------------------------------------------------------- 8. the command-line tools

def _lines(e_log, ch, Fs):
    """a channel's log as the tools print it: rtl_fsk -L's columns without the wall clock, the channel in front"""
    out = []
    for e in e_log:
        S, N = float(e["S"]), float(e["N"])
        out.append("%d: Rx frame src: 0x%02x seq: %3d S: %e N: %e SNR: %5.2f dB t_rx: %.4f s"
                   % (ch, e["source"], e["seq"], S, N, 10.0 * math.log10(S / (N + 1e-30) + 1e-30), int(e["t_samples"]) / float(Fs)))
    return out


def _modem_args():
    lp = ms.LOOP
    return ["--code", ms.CODE, "-s", str(lp["Fs"]), "-a", str(lp["mFs"]), "-r", str(lp["Rs"]), "-m", str(lp["M"]), "--fsk_lower", str(lp["est_min"]),
            "--fsk_upper", str(lp["est_max"]), "-q", "-c", ",".join(map(str, lp["offsets"]))]


def _tx_args(block):
    lp = ms.LOOP
    return ["--f1", str(lp["f1"]), "--shift", str(lp["shift"]), "--gains", ",".join(f"{g:.9g}" for g in ms.LOOP_GAINS), "--gap", str(LOOP_GAP),
            "--block", str(block), "--queue", str(50 + lp["nframes"] * 544 + LOOP_GAP)]


def _ping_cli(src, dst, block):
    cmd = [os.path.join(ms.BIN, "ping_channels")] + _modem_args() + _tx_args(block) + \
          ["--source", "1", "--filter", "1", "--frames", str(ms.LOOP["nframes"]), "--period", "1", "--first", ",".join(map(str, FIRST)), "--bursts", "1",
           "--seq", "--log-entries", "16", "-i", src, "-o", dst]
    p = subprocess.run(cmd, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    return np.fromfile(dst, dtype=np.uint8), p.stderr.decode().splitlines()


def test_cli_tools_equal_the_binding(loop, tmp_path):
    """The closed loop again, through files: each tool reads the other's output behind one block of silence, which is the loop's delay."""
    import torch
    import pirip_amd
    lp = ms.LOOP
    block, blk = loop["term"].block, loop["term"].block * 2
    t_out, r_out = loop["t_out"].cpu().numpy().reshape(-1), loop["r_out"].cpu().numpy().reshape(-1)
    silence = np.full(blk, 128, np.uint8)
    name = {k: str(tmp_path / k) for k in ("silence", "t", "t_delayed", "r", "r_delayed", "t2", "payloads")}
    # ping_channels on silence: what it sends does not depend on what it hears
    np.tile(silence, LOOP_CALLS).tofile(name["silence"])
    got, lines = _ping_cli(name["silence"], name["t"], block)
    assert got.size == t_out.size and np.array_equal(got, t_out)
    assert [ln for ln in lines if "Rx frame" in ln] == []
    assert lines == ["%d: bursts 1 frames sent 3 received 0 PER 1.000" % c for c in range(4)]
    # ... through frame_repeater_channels ...
    np.concatenate([silence, got[:-blk]]).tofile(name["t_delayed"])
    cmd = [os.path.join(ms.BIN, "frame_repeater_channels")] + _modem_args() + _tx_args(block) + \
          ["--source", "2", "--filter", "2", "--route", ",".join(map(str, ROUTE)), "--holdoff", "1", "--max-burst", str(lp["nframes"]),
           "--pending", str(lp["nframes"] + 1), "-i", name["t_delayed"], "-o", name["r"]]
    p = subprocess.run(cmd, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    back = np.fromfile(name["r"], dtype=np.uint8)
    assert back.size == r_out.size and np.array_equal(back, r_out)
    # ... and back into ping_channels: the loop's log, line by line, and no frame lost
    np.concatenate([silence, back[:-blk]]).tofile(name["r_delayed"])
    got2, lines = _ping_cli(name["r_delayed"], name["t2"], block)
    assert np.array_equal(got2, t_out)
    for ch in range(4):
        assert [ln for ln in lines if ln.startswith("%d: Rx frame" % ch)] == _lines(loop["logs"][ch], ch, lp["mFs"]), ch
    assert lines[-4:] == ["%d: bursts 1 frames sent 3 received 3 PER 0.000" % c for c in range(4)] and len(lines) == 16
    # rtl_fsk_channels -L on the repeater's output, against a logger-only HipPing behind a receiver of that tool's block size
    wide = lp["Fs"] // 4 // lp["D"] * lp["D"]
    assert back.size % (wide * 2) == 0
    p = subprocess.run([os.path.join(ms.BIN, "rtl_fsk_channels")] + _modem_args() + ["-L", "-i", name["r"], "-o", name["payloads"]], capture_output=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    from test_mux import _rx_handles
    dem, ld, ch_ = _rx_handles()
    rx = pirip_amd.HipRx(dem, ldpc=ld, chan=ch_, block=wide)
    logger = pirip_amd.HipPing(rx=rx, log_entries=16)
    d_back = torch.from_numpy(back).cuda()
    for k in range(back.size // (wide * 2)):
        logger.push(d_back.data_ptr() + k * wide * 2, wide * 2)
    assert logger.counters()["frames"].tolist() == [lp["nframes"]] * 4
    lines = p.stderr.decode().splitlines()
    for ch in range(4):
        assert [ln for ln in lines if ln.startswith("%d: Rx frame" % ch)] == _lines(logger.log(ch), ch, lp["mFs"]), ch
    assert len(lines) == 12
    for ch in range(4):
        assert os.path.getsize(name["payloads"] + ".%d" % ch) == lp["nframes"] * pingref.KB
